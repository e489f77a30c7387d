// msc.hip -- Masked Scene Contrast pretraining (pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py): the three
// stretches of the wrapper around the backbone.
//
// 1  Radius-bounded nearest matches (match_contrastive_pair, :144-162).  For a query of view 1 the up-to-k (k <= PTC_MSC_MAX_K) points of the same
//    scene of view 2 with fp32 sqrt(d2) < max_radius, ascending (d2, index): exactly ptc_knn_query(8, ...) followed by the reference's
//    `distance < max_radius` ("k nearest, then filter" and "filter, then k nearest" pick the same set).  d2 is pointops.hip's unfused
//    expression and the root is taken as ptc_knn_query takes it.  View 2 is sorted (ptc_sort_keys, stable: ascending index inside a
//    cell) into a grid of cells of edge >= max_radius * (1 + 1e-4), grown when the extent would overflow the 16-bit cell fields; a query
//    visits its 27 cells and keeps its candidates in registers as a sorted list.  A non-finite coordinate matches nothing.  The number
//    of matched queries and the largest count are reduced per wave and added with INTEGER atomics.
// 2  Pair selection (:154-169): the j-th matched query q (ascending) takes candidate count - 1 - r[j] % count of its list.
// 3  Cross-mask patches (generate_cross_masks, :94-128): the linearised ids of voxel_grid(pos = floored cells, size 1, batch, start 0)
//    -- num = trunc(max) + 1 per axis, negative cells and their collisions included -- sorted as signed numbers; run boundaries ->
//    ranks (torch.unique's sorted numbering) -> point_mask[i] = patch_mask[rank[i]].
// 4  Fused InfoNCE (compute_contrastive_loss, :174-203).  Matched rows are gathered and normalised (x / (|x| + 1e-7)); S = A B^T is
//    formed 16 x 16 at a time on v_mfma_f32_16x16x4_f32 (layout notes in attention_rpe_f32.h) and never stored: the forward keeps an
//    online log-sum-exp of S / t, the row sums and the diagonal; the backward recomputes the tiles from the saved lse and forms
//    dA = (softmax - I) B / (P t) and dB = (softmax - I)^T A / (P t), then applies the Jacobian of the normalisation.  Rows matched
//    several times are summed after a stable sort by row, in that order.  No float atomics; every reduction has a fixed order, so
//    forward and backward are bit-reproducible.
// 5  Partitioned InfoNCE of MSC-v1m2 (masked_scene_contrast_v1m2_csc.py:182-264): 4 per scene and per partition class of the logit,
//    on pairs grouped by scene; notes at the section.
#include "cell_grid.h"
#include "mma.h"

#define MSC_THREADS 256
#define MSC_KMAX PTC_MSC_MAX_K

namespace {

// smallest i with p < ends[i]; b when p >= ends[b-1]
__device__ __forceinline__ int msc_scene_of(const int* __restrict__ ends, int b, int64_t p) {
  int lo = 0, hi = b;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (p < ends[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}
int msc_grid1(int64_t n) { return (int)ptc_cdiv(n > 0 ? n : 1, MSC_THREADS); }

// ---------------------------------------------------------------------------------------------------------------------------------
// 1. matching
// ---------------------------------------------------------------------------------------------------------------------------------
// key of a row of `xyz` (scene from `offset`); scene `b` = matches nothing (non-finite, or beyond the last offset).  Also zeroes the two
// counters that msc_match_kernel adds to.
__global__ void msc_keys_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ offset, int b, int64_t n,
                                const PtcCellGrid* __restrict__ g, int64_t* __restrict__ keys, int32_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == 0) { stats[0] = 0; stats[1] = 0; }
  const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
  const int s = msc_scene_of(offset, b, i);
  if (!ptc_finite3(x, y, z) || s >= b) {
    keys[i] = ptc_cell_key(b, 0, 0, 0);
    return;
  }
  const double e = g->edge;
  keys[i] = ptc_cell_key(s, ptc_cell(x, g->mn[0], e), ptc_cell(y, g->mn[1], e), ptc_cell(z, g->mn[2], e));
}

// one query per thread: the 9 x-runs of its 27 cells, candidates kept as a register list ascending by (d2, index)
__global__ void __launch_bounds__(MSC_THREADS)
msc_match_kernel(const float* __restrict__ qxyz, const int32_t* __restrict__ qoffset, int b, int64_t m, const PtcCellGrid* __restrict__ g,
                 const int64_t* __restrict__ skeys, const float4* __restrict__ sxyz, int64_t n, int k, float radius,
                 int32_t* __restrict__ count, int32_t* __restrict__ cand, int32_t* __restrict__ stats) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float bd[MSC_KMAX];
  int bi[MSC_KMAX];
#pragma unroll
  for (int j = 0; j < MSC_KMAX; ++j) { bd[j] = INFINITY; bi[j] = -1; }
  int cnt = 0;
  if (q < m) {
    const float qx = qxyz[q * 3], qy = qxyz[q * 3 + 1], qz = qxyz[q * 3 + 2];
    const int s = msc_scene_of(qoffset, b, q);
    if (ptc_finite3(qx, qy, qz) && s < b && n > 0) {
      const double e = g->edge;
      const int cx = ptc_cell(qx, g->mn[0], e), cy = ptc_cell(qy, g->mn[1], e), cz = ptc_cell(qz, g->mn[2], e);
      ptc_cell_runs(skeys, n, s, cx, cy, cz, [&](int64_t lo, int64_t hi, int, int) {
        for (int64_t p = lo; p < hi; ++p) {
          const float4 c = sxyz[p];
          const float d2 = ptc_dist2(qx, qy, qz, c.x, c.y, c.z);
          if (!((float)sqrt((double)d2) < radius)) continue;
          const int ci = __float_as_int(c.w);
          if (d2 < bd[MSC_KMAX - 1] || (d2 == bd[MSC_KMAX - 1] && ci < bi[MSC_KMAX - 1]) || bi[MSC_KMAX - 1] < 0) {
            int pos = 0;
#pragma unroll
            for (int j = 0; j < MSC_KMAX; ++j) pos += (bi[j] >= 0 && (bd[j] < d2 || (bd[j] == d2 && bi[j] < ci))) ? 1 : 0;
#pragma unroll
            for (int j = MSC_KMAX - 1; j > 0; --j)
              if (j > pos) { bd[j] = bd[j - 1]; bi[j] = bi[j - 1]; }
#pragma unroll
            for (int j = 0; j < MSC_KMAX; ++j)
              if (j == pos) { bd[j] = d2; bi[j] = ci; }
            cnt += cnt < MSC_KMAX ? 1 : 0;
          }
        }
      });
    }
    cnt = cnt < k ? cnt : k;
    count[q] = cnt;
#pragma unroll
    for (int j = 0; j < MSC_KMAX; ++j)
      if (j < k) cand[q * k + j] = j < cnt ? bi[j] : -1;
  }
  // every lane arrives here: matched queries and the largest count of the wave, then two integer atomics
  const unsigned long long mask = __ballot(cnt > 0);
  int mx = cnt;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int other = __shfl_xor(mx, o, 64);
    mx = other > mx ? other : mx;
  }
  if (ptc_lane() == 0 && mask != 0ull) {
    atomicAdd(stats, (int32_t)__popcll(mask));
    atomicMax(stats + 1, (int32_t)mx);
  }
}

__global__ void msc_zero_match_kernel(int64_t m, int k, int32_t* __restrict__ count, int32_t* __restrict__ cand, int32_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { stats[0] = 0; stats[1] = 0; }
  if (i < m) count[i] = 0;
  if (i < m * k) cand[i] = -1;
}

struct MatchLayout {
  PtcCellGridLayout g;
  size_t total;
};
MatchLayout match_layout(int64_t n) {
  MatchLayout Y;
  PtcArena A;
  const int64_t c = n > 0 ? n : 1;
  Y.g.take_arrays(A, c);
  Y.g.take_scratch(A, c);
  Y.total = A.total;
  return Y;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 2. pair selection
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void msc_flags_kernel(const int32_t* __restrict__ count, int64_t m, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) flag[i] = count[i] > 0 ? 1 : 0;
}
__global__ void msc_select_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ cand, const int64_t* __restrict__ rank,
                                  int64_t m, int k, const int64_t* __restrict__ r, int64_t n_matched, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int c = count[i];
  const int64_t j = rank[i];
  if (c <= 0 || c > k || j >= n_matched) return;
  int64_t t = r[j] % c;
  t = t < 0 ? t + c : t;          // torch's remainder takes the divisor's sign
  out[j * 2] = i;
  out[j * 2 + 1] = cand[i * k + (c - 1 - (int)t)];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3. cross-mask patches
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void msc_cell_max_kernel(const float* __restrict__ c1, int64_t n1, const float* __restrict__ c2, int64_t n2, uint32_t* __restrict__ mx) {
  uint32_t hi[3] = {0u, 0u, 0u};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += (int64_t)gridDim.x * blockDim.x) {
    const float* p = i < n1 ? c1 + i * 3 : c2 + (i - n1) * 3;
    for (int a = 0; a < 3; ++a) {
      const uint32_t e = ptc_float_enc(p[a]);
      hi[a] = e > hi[a] ? e : hi[a];
    }
  }
  for (int a = 0; a < 3; ++a)
    if (hi[a] != 0u) atomicMax(mx + a, hi[a]);
}

// id = sum_a cell_a * stride_a, stride = (1, num_x, num_x num_y, num_x num_y num_z), num = trunc(max) + 1, batch the slowest; stored with
// the sign bit flipped so that the unsigned radix sort orders the ids as signed numbers
__global__ void msc_patch_ids_kernel(const float* __restrict__ c1, const int32_t* __restrict__ off1, int64_t n1, const float* __restrict__ c2,
                                     const int32_t* __restrict__ off2, int64_t n2, int b, const uint32_t* __restrict__ mx,
                                     int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1 + n2) return;
  const bool first = i < n1;
  const float* p = first ? c1 + i * 3 : c2 + (i - n1) * 3;
  int s = first ? msc_scene_of(off1, b, i) : msc_scene_of(off2, b, i - n1);
  s = s < b ? s : b - 1;
  const uint64_t nx = (uint64_t)((int64_t)ptc_float_dec(mx[0]) + 1), ny = (uint64_t)((int64_t)ptc_float_dec(mx[1]) + 1), nz = (uint64_t)((int64_t)ptc_float_dec(mx[2]) + 1);
  // two's-complement wrap-around as the int64 tensor arithmetic of voxel_grid
  const uint64_t id = (uint64_t)(int64_t)p[0] + (uint64_t)(int64_t)p[1] * nx + (uint64_t)(int64_t)p[2] * (nx * ny) + (uint64_t)(int64_t)s * (nx * ny * nz);
  keys[i] = (int64_t)(id ^ 0x8000000000000000ull);
}

__global__ void msc_run_flags_kernel(const int64_t* __restrict__ skeys, int64_t n, int32_t* __restrict__ flag) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) flag[p] = (p > 0 && skeys[p] != skeys[p - 1]) ? 1 : 0;
}
// rank of sorted position p = number of run boundaries up to and including p
__global__ void msc_ranks_kernel(const int32_t* __restrict__ flag, const int64_t* __restrict__ scan, const int64_t* __restrict__ order, int64_t n,
                                 int32_t* __restrict__ cluster, int64_t* __restrict__ patch_num) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t rank = scan[p] + flag[p];
  cluster[order[p]] = (int32_t)rank;
  if (p == n - 1) patch_num[0] = rank + 1;
}
__global__ void msc_patch_masks_kernel(const int32_t* __restrict__ cluster, const int32_t* __restrict__ patch_mask, int64_t patch_num,
                                       int64_t n1, int64_t n2, uint8_t* __restrict__ mask1, uint8_t* __restrict__ mask2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1 + n2) return;
  const int c = cluster[i];
  const int tag = (c >= 0 && c < patch_num) ? patch_mask[c] : 0;
  if (i < n1) mask1[i] = tag == 1 ? 1 : 0;      // view 1 keeps tag 1, view 2 keeps tag 2 (:139-140)
  else mask2[i - n1] = tag == 2 ? 1 : 0;
}

struct PatchLayout {
  size_t mx, keys, order, skeys, flag, scan, scratch, total;
};
PatchLayout patch_layout(int64_t n) {
  PatchLayout Y;
  PtcArena A;
  const int64_t c = n > 0 ? n : 1;
  Y.mx = A.take(3 * 4);
  Y.keys = A.take((size_t)c * 8);
  Y.order = A.take((size_t)c * 8);
  Y.skeys = A.take((size_t)c * 8);
  Y.flag = A.take((size_t)c * 4);
  Y.scan = A.take((size_t)c * 8);
  const size_t s1 = ptc_sort_keys_workspace_bytes(c, 1), s2 = ptc_exclusive_scan_workspace_bytes(c);
  Y.scratch = A.take(s1 > s2 ? s1 : s2);
  Y.total = A.total;
  return Y;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// 4. InfoNCE
// ---------------------------------------------------------------------------------------------------------------------------------
// (outside the unnamed namespace: the dynamic-LDS array `smem` is a name of the global one)
#define NCE_ROWS 64                  // stationary rows of a workgroup: 16 per wave
#define NCE_TILE 64                  // streamed rows staged in LDS at a time
#define NCE_MAX_SPLIT 8
#define NCE_EPS 1e-7f
#define NCE_MAX_P (1 << 20)          // the O(P^2) products and the one-workgroup finish are meant for P of this order, not for 2^31

__device__ __forceinline__ f32x4 nce_splat(float v) { return (f32x4){v, v, v, v}; }

// S / t as ONE rounded product in the forward and in the backward alike: contracted into the subtraction of the lse it would differ
// from the value the lse was built from, and exp(z - lse) of a one-column row would not be exactly 1
__device__ __forceinline__ float nce_logit(float s, float inv_t) {
#pragma clang fp contract(off)
  const float z = s * inv_t;
  return z;
}

// one wave per matched row: y = x / (|x| + 1e-7) of feat[index[p * 2 + side]]; an index outside [0, n_rows) gives a zero row
__global__ void __launch_bounds__(MSC_THREADS)
nce_gather_norm_kernel(const float* __restrict__ feat, int64_t n_rows, const int64_t* __restrict__ match, int side, int64_t P, int C,
                       float* __restrict__ y, float* __restrict__ norm) {
  const int64_t p = (int64_t)blockIdx.x * (MSC_THREADS / 64) + (threadIdx.x >> 6);
  const int lane = ptc_lane();
  const bool live = p < P;
  const int64_t row = live ? match[p * 2 + side] : -1;
  const bool ok = row >= 0 && row < n_rows;
  float ss = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = ok ? feat[row * C + c] : 0.f;
    ss += v * v;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float nrm = sqrtf(ss);
  if (!live) return;
  for (int c = lane; c < C; c += 64) y[p * C + c] = ok ? feat[row * C + c] / (nrm + NCE_EPS) : 0.f;
  if (lane == 0) norm[p] = nrm;
}

// rows [r0, r0 + NCE_TILE) of src [P][C] into the LDS image [NCE_TILE][LDW] (zeros beyond P and beyond C)
__device__ __forceinline__ void nce_stage(const float* __restrict__ src, int64_t r0, int64_t P, int C, int LDW, float* img) {
  const int per_row = LDW >> 2;
  for (int i = threadIdx.x; i < NCE_TILE * per_row; i += MSC_THREADS) {
    const int row = i / per_row, c4 = (i - row * per_row) * 4;
    f32x4 v = nce_splat(0.f);
    if (r0 + row < P && c4 < C) v = *reinterpret_cast<const f32x4*>(src + (r0 + row) * C + c4);
    *reinterpret_cast<f32x4*>(img + row * LDW + c4) = v;
  }
}

// S^T sub-tile: lane (j, g) gets S(stationary row j, streamed rows 16 t + 4 g + r), r = 0..3
template <int CH>
__device__ __forceinline__ f32x4 nce_scores(const float* img, int LDW, int t, int j, int g, const f32x4 (&stat)[CH]) {
  f32x4 s = nce_splat(0.f);
  const float* row = img + (16 * t + j) * LDW + 4 * g;
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(row + 16 * ch);
    s = ptc_mfma_f32_4(a[0], stat[ch][0], s);
    s = ptc_mfma_f32_4(a[1], stat[ch][1], s);
    s = ptc_mfma_f32_4(a[2], stat[ch][2], s);
    s = ptc_mfma_f32_4(a[3], stat[ch][3], s);
  }
  return s;
}

// forward: grid (row blocks, column splits).  Per stationary row and split: running max and sum of exp(S / t - max), the sum of S, and
// (from the one lane that meets it) the diagonal.  part [split][P][3].
template <int CH>
__global__ void __launch_bounds__(MSC_THREADS)
nce_fwd_kernel(const float* __restrict__ A, const float* __restrict__ B, int64_t P, int C, float inv_t, int tiles_per_split,
               float* __restrict__ part, float* __restrict__ diag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* img = reinterpret_cast<float*>(smem);
  constexpr int LDW = 16 * CH + 4;
  const int lane = ptc_lane(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int64_t sr = (int64_t)blockIdx.x * NCE_ROWS + wave * 16 + j;
  f32x4 stat[CH];
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    const int c = 16 * ch + 4 * g;
    stat[ch] = (sr < P && c < C) ? *reinterpret_cast<const f32x4*>(A + sr * C + c) : nce_splat(0.f);
  }
  const int64_t n_tiles = (P + NCE_TILE - 1) / NCE_TILE;
  const int64_t t_lo = (int64_t)blockIdx.y * tiles_per_split;
  const int64_t t_hi = t_lo + tiles_per_split < n_tiles ? t_lo + tiles_per_split : n_tiles;
  float m = -INFINITY, l = 0.f, rs = 0.f;
  for (int64_t tile = t_lo; tile < t_hi; ++tile) {
    __syncthreads();
    nce_stage(B, tile * NCE_TILE, P, C, LDW, img);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NCE_TILE / 16; ++t) {
      const f32x4 s = nce_scores<CH>(img, LDW, t, j, g, stat);
      float z[4], mt = m;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t col = tile * NCE_TILE + 16 * t + 4 * g + r;
        const bool cv = col < P;
        z[r] = cv ? nce_logit(s[r], inv_t) : -INFINITY;
        rs += cv ? s[r] : 0.f;
        mt = fmaxf(mt, z[r]);
        if (cv && col == sr) diag[sr] = s[r];
      }
      if (mt != -INFINITY) {
        l *= __expf(m - mt);             // m = -inf: l is 0 and exp(-inf) = 0
        m = mt;
#pragma unroll
        for (int r = 0; r < 4; ++r) l += __expf(z[r] - m);
      }
    }
  }
  // the four lanes of a row (g = 0..3), merged in a fixed order
  float M = fmaxf(m, __shfl_xor(m, 16, 64));
  M = fmaxf(M, __shfl_xor(M, 32, 64));
  float lw = m == -INFINITY ? 0.f : l * __expf(m - M);
  const float l1 = __shfl_xor(lw, 16, 64), r1 = __shfl_xor(rs, 16, 64);
  // lanes g and g ^ 1 add the same two values; then the pairs (0,1) + (2,3) in that order on every lane
  float lp = (g & 1) ? l1 + lw : lw + l1, rp = (g & 1) ? r1 + rs : rs + r1;
  const float l2 = __shfl_xor(lp, 32, 64), r2 = __shfl_xor(rp, 32, 64);
  const float L = (g & 2) ? l2 + lp : lp + l2, R = (g & 2) ? r2 + rp : rp + r2;
  if (g == 0 && sr < P) {
    float* o = part + ((int64_t)blockIdx.y * P + sr) * 3;
    o[0] = M;
    o[1] = L;
    o[2] = R;
  }
}

// one workgroup: merges the splits of every row in order, writes lse, then the three means (double accumulators, fixed tree).
// P / 256 rows per thread: 32 at the config's matching_max_pair = 8192 (a few microseconds); the entry points accept P <= NCE_MAX_P
__global__ void __launch_bounds__(MSC_THREADS)
nce_finish_kernel(const float* __restrict__ part, const float* __restrict__ diag, int64_t P, int n_split, float inv_t,
                  float* __restrict__ lse, float* __restrict__ out) {
  __shared__ double red[3][MSC_THREADS];
  double a_loss = 0.0, a_pos = 0.0, a_all = 0.0;
  for (int64_t i = threadIdx.x; i < P; i += MSC_THREADS) {
    float M = -INFINITY;
    for (int s = 0; s < n_split; ++s) M = fmaxf(M, part[((int64_t)s * P + i) * 3]);
    float L = 0.f, R = 0.f;
    for (int s = 0; s < n_split; ++s) {
      const float* p = part + ((int64_t)s * P + i) * 3;
      L += p[1] * __expf(p[0] - M);
      R += p[2];
    }
    const float v = M + __logf(L);
    lse[i] = v;
    a_loss += (double)(v - diag[i] * inv_t);
    a_pos += (double)diag[i];
    a_all += (double)(R / (float)P);
  }
  red[0][threadIdx.x] = a_loss;
  red[1][threadIdx.x] = a_pos;
  red[2][threadIdx.x] = a_all;
  __syncthreads();
  for (int o = MSC_THREADS / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int a = 0; a < 3; ++a) red[a][threadIdx.x] += red[a][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float pos = (float)(red[1][0] / (double)P);
    out[0] = (float)(red[0][0] / (double)P);
    out[1] = pos;
    out[2] = (float)(red[2][0] / (double)P) - pos / (float)P;     // :191, as written there
  }
}

// backward products: blockIdx.y = 0: stationary A rows, dA = G B;  1: stationary B rows, dB = G^T A, with
// G[i][j] = (exp(S_ij / t - lse_i) - [i == j]) * gs, gs = dloss / (P t).  `lse` always belongs to the A side.
template <int CH>
__global__ void __launch_bounds__(MSC_THREADS)
nce_bwd_kernel(const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ lse, const float* __restrict__ dloss,
               int64_t P, int C, float inv_t, float* __restrict__ gA, float* __restrict__ gB) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* img = reinterpret_cast<float*>(smem);
  constexpr int LDW = 16 * CH + 4;
  float* lse_t = img + NCE_TILE * LDW;
  const bool role_b = blockIdx.y != 0;
  const float* S_ = role_b ? B : A;          // stationary
  const float* T_ = role_b ? A : B;          // streamed
  float* out = role_b ? gB : gA;
  const int lane = ptc_lane(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int64_t sr = (int64_t)blockIdx.x * NCE_ROWS + wave * 16 + j;
  const float gs = dloss[0] * inv_t / (float)P;
  f32x4 stat[CH], acc[CH];
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    const int c = 16 * ch + 4 * g;
    stat[ch] = (sr < P && c < C) ? *reinterpret_cast<const f32x4*>(S_ + sr * C + c) : nce_splat(0.f);
    acc[ch] = nce_splat(0.f);
  }
  const float lse_s = (!role_b && sr < P) ? lse[sr] : 0.f;
  const int64_t n_tiles = (P + NCE_TILE - 1) / NCE_TILE;
  for (int64_t tile = 0; tile < n_tiles; ++tile) {
    __syncthreads();
    nce_stage(T_, tile * NCE_TILE, P, C, LDW, img);
    if (threadIdx.x < NCE_TILE) {
      const int64_t r = tile * NCE_TILE + threadIdx.x;
      lse_t[threadIdx.x] = (role_b && r < P) ? lse[r] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NCE_TILE / 16; ++t) {
      const f32x4 s = nce_scores<CH>(img, LDW, t, j, g, stat);
      f32x4 w;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t tr = tile * NCE_TILE + 16 * t + 4 * g + r;
        const float ls = role_b ? lse_t[16 * t + 4 * g + r] : lse_s;
        const float p = __expf(nce_logit(s[r], inv_t) - ls) - (tr == sr ? 1.f : 0.f);
        w[r] = (tr < P && sr < P) ? p * gs : 0.f;
      }
      // acc[channels 16 ch + 4 g ..][row j] += sum over the 16 streamed rows: lane (c', k) reads column c' of rows 4 k + r
      const float* col = img + (16 * t + 4 * g) * LDW + j;
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) {
        acc[ch] = ptc_mfma_f32_4(col[16 * ch], w[0], acc[ch]);
        acc[ch] = ptc_mfma_f32_4(col[16 * ch + LDW], w[1], acc[ch]);
        acc[ch] = ptc_mfma_f32_4(col[16 * ch + 2 * LDW], w[2], acc[ch]);
        acc[ch] = ptc_mfma_f32_4(col[16 * ch + 3 * LDW], w[3], acc[ch]);
      }
    }
  }
  if (sr < P) {
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
      const int c = 16 * ch + 4 * g;
      if (c < C) *reinterpret_cast<f32x4*>(out + sr * C + c) = acc[ch];
    }
  }
}

// Jacobian of y = x / (n + eps), n = |x|, in place on the gradient: dx = (gy - y (gy . y) (n + eps) / n) / (n + eps); n = 0: dx = gy / eps
// (torch's norm backward is 0 there).  One wave per row, fixed-order dot.
__global__ void __launch_bounds__(MSC_THREADS)
nce_norm_bwd_kernel(const float* __restrict__ y, const float* __restrict__ norm, int64_t P, int C, float* __restrict__ gy) {
  const int64_t p = (int64_t)blockIdx.x * (MSC_THREADS / 64) + (threadIdx.x >> 6);
  const int lane = ptc_lane();
  const bool live = p < P;
  float dot = 0.f;
  for (int c = lane; c < C; c += 64) dot += live ? gy[p * C + c] * y[p * C + c] : 0.f;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) dot += __shfl_xor(dot, o, 64);
  if (!live) return;
  const float n = norm[p], ne = n + NCE_EPS;
  const float k = n > 0.f ? dot * ne / n : 0.f;
  for (int c = lane; c < C; c += 64) gy[p * C + c] = (gy[p * C + c] - y[p * C + c] * k) / ne;
}

__global__ void nce_row_keys_kernel(const int64_t* __restrict__ match, int side, int64_t P, int64_t n_rows, int64_t* __restrict__ keys) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int64_t row = match[p * 2 + side];
  keys[p] = (row >= 0 && row < n_rows) ? row : n_rows;      // n_rows: dropped
}
// dfeat[row] = sum of dx over the run of `row` in the stable order (ascending pair index); one thread per (run start, float4)
__global__ void nce_segment_add_kernel(const int64_t* __restrict__ skeys, const int64_t* __restrict__ order, const float* __restrict__ dx,
                                       int64_t P, int C, int64_t n_rows, float* __restrict__ dfeat) {
  const int c4n = C >> 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * c4n) return;
  const int64_t p = i / c4n;
  const int c = (int)(i - p * c4n) * 4;
  const int64_t row = skeys[p];
  if (row >= n_rows || (p > 0 && skeys[p - 1] == row)) return;
  f32x4 s = nce_splat(0.f);
  for (int64_t q = p; q < P && skeys[q] == row; ++q) s += *reinterpret_cast<const f32x4*>(dx + order[q] * C + c);
  *reinterpret_cast<f32x4*>(dfeat + row * C + c) = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 5. Partitioned InfoNCE (MSC-v1m2, masked_scene_contrast_v1m2_csc.py:182-252)
// ---------------------------------------------------------------------------------------------------------------------------------
// The pairs are sorted by scene (stable), so a scene is a range of rows AND of columns of S = A B^T and a block of 64 stationary rows
// streams only the column tiles that meet the scenes of its rows; "same scene" stays a per-element test, so a block may straddle a
// boundary.  Every logit (i, j) has one of five classes, computed from the coordinates staged with the tile and never stored; a
// row keeps one online log-sum-exp per class over its off-diagonal members, and the diagonal joins each of them in the finish.
#define CSC_CLASSES 5
#define CSC_PART 16                  // words per (split, row): max [5], sum [5], member counts [5] (int32), row sum of S
#define CSC_MAX_SCENES 32766

// class of the logit (row i, column j) from a = x1[j] and b = x2[i]: rel = a - b is the reference's transposition (:186 builds
// coord1.unsqueeze(0) - coord2.unsqueeze(1) and indexes it like sim).  0 / 1: r1 < d <= r2 above / below, 2 / 3: d > r2 above / below,
// 4: the rest (d <= r1, rel.z == 0, anything not a number).  No contraction: the forward, both roles of the backward and the finish
// must see the same rounded d, as nce_logit's callers must see the same z.
__device__ __forceinline__ int csc_class(float ax, float ay, float az, float bx, float by, float bz, float r1, float r2) {
#pragma clang fp contract(off)
  const float rx = ax - bx, ry = ay - by, rz = az - bz;
  const float d = sqrtf(((rx * rx + ry * ry) + rz * rz) + 1e-7f);
  const bool far = d > r2, mid = d > r1 && d <= r2, up = rz > 0.f, down = rz < 0.f;
  if (!(far || mid) || !(up || down)) return 4;
  return (far ? 2 : 0) + (down ? 1 : 0);
}

// scene of a pair = scene of its view-1 row; nb: dropped (an index outside its matrix or beyond the last offset)
__global__ void csc_scene_keys_kernel(const int64_t* __restrict__ match, int64_t P, int64_t n1, int64_t n2, const int32_t* __restrict__ offset,
                                      int nb, int64_t* __restrict__ keys) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int64_t a = match[p * 2], b = match[p * 2 + 1];
  keys[p] = (a >= 0 && a < n1 && b >= 0 && b < n2) ? msc_scene_of(offset, nb, a) : nb;
}

// the pairs in scene order: smatch[q] = match[order[q]]; xs1[q] = (x1 of the pair, scene bits), xs2[q] = (x2, scene bits);
// start[b] = the first position whose scene is >= b, for b = 0 .. nb + 1 (start[nb + 1] = P)
__global__ void csc_group_kernel(const int64_t* __restrict__ match, const int64_t* __restrict__ order, const int64_t* __restrict__ skeys, int64_t P,
                                 const float* __restrict__ coord1, const float* __restrict__ coord2, int nb, int64_t* __restrict__ smatch,
                                 float4* __restrict__ xs1, float4* __restrict__ xs2, int32_t* __restrict__ start) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P) return;
  const int64_t o = order[q];
  const int s = (int)skeys[q];
  const int64_t a = match[o * 2], b = match[o * 2 + 1];
  smatch[q * 2] = a;
  smatch[q * 2 + 1] = b;
  float4 u, v;
  u.x = u.y = u.z = v.x = v.y = v.z = 0.f;
  u.w = v.w = __int_as_float(s);
  if (s < nb) {
    u.x = coord1[a * 3], u.y = coord1[a * 3 + 1], u.z = coord1[a * 3 + 2];
    v.x = coord2[b * 3], v.y = coord2[b * 3 + 1], v.z = coord2[b * 3 + 2];
  }
  xs1[q] = u;
  xs2[q] = v;
  const int prev = q > 0 ? (int)skeys[q - 1] : -1;
  for (int k = prev + 1; k <= s; ++k) start[k] = (int32_t)q;
  if (q == P - 1)
    for (int k = s + 1; k <= nb + 1; ++k) start[k] = (int32_t)P;
}

// the column tiles [t_lo, t_hi) a block of stationary rows has to stream: those that meet the scenes of its first and last row
__device__ __forceinline__ void csc_tile_range(const float4* __restrict__ xs, const int32_t* __restrict__ start, int64_t P, int nb,
                                               int64_t& t_lo, int64_t& t_hi) {
  const int64_t r0 = (int64_t)blockIdx.x * NCE_ROWS;
  const int64_t rl = (r0 + NCE_ROWS < P ? r0 + NCE_ROWS : P) - 1;
  const int s_lo = __float_as_int(xs[r0].w), s_hi = __float_as_int(xs[rl].w);
  t_lo = t_hi = 0;
  if (s_lo >= nb) return;                                  // dropped pairs only
  t_lo = start[s_lo] / NCE_TILE;
  t_hi = ((int64_t)start[s_hi + 1] + NCE_TILE - 1) / NCE_TILE;
}

// the (max, sum) pairs of the four lanes of a row (g = 0..3), merged in the fixed order of nce_fwd_kernel
__device__ __forceinline__ void csc_merge4(float& m, float& l, int g) {
  float M = fmaxf(m, __shfl_xor(m, 16, 64));
  M = fmaxf(M, __shfl_xor(M, 32, 64));
  const float lw = m == -INFINITY ? 0.f : l * __expf(m - M);
  const float l1 = __shfl_xor(lw, 16, 64);
  const float lp = (g & 1) ? l1 + lw : lw + l1;
  const float l2 = __shfl_xor(lp, 32, 64);
  l = (g & 2) ? l2 + lp : lp + l2;
  m = M;
}

// forward: grid (row blocks, column splits of the block's own tile range).  Per stationary row and split: for each class the running
// max and sum of exp(S / t - max) over its off-diagonal members of the row's scene and their number (the diagonal counted by its
// class), the sum of S over the scene, and the diagonal.  part [split][P][CSC_PART].
template <int CH>
__global__ void __launch_bounds__(MSC_THREADS)
csc_fwd_kernel(const float* __restrict__ A, const float* __restrict__ B, const float4* __restrict__ xs1, const float4* __restrict__ xs2,
               const int32_t* __restrict__ start, int64_t P, int C, int nb, float inv_t, float r1, float r2, float* __restrict__ part,
               float* __restrict__ diag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* img = reinterpret_cast<float*>(smem);
  constexpr int LDW = 16 * CH + 4;
  float4* xt = reinterpret_cast<float4*>(img + NCE_TILE * LDW);
  const int lane = ptc_lane(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int64_t sr = (int64_t)blockIdx.x * NCE_ROWS + wave * 16 + j;
  f32x4 stat[CH];
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    const int c = 16 * ch + 4 * g;
    stat[ch] = (sr < P && c < C) ? *reinterpret_cast<const f32x4*>(A + sr * C + c) : nce_splat(0.f);
  }
  float4 me;
  me.x = me.y = me.z = 0.f;
  me.w = __int_as_float(nb);
  if (sr < P) me = xs2[sr];
  const int my_scene = __float_as_int(me.w);
  const bool row_ok = sr < P && my_scene < nb;
  int64_t T_lo, T_hi;
  csc_tile_range(xs2, start, P, nb, T_lo, T_hi);
  const int64_t per_split = (T_hi - T_lo + gridDim.y - 1) / gridDim.y;
  const int64_t t_lo = T_lo + (int64_t)blockIdx.y * per_split;
  const int64_t t_hi = t_lo + per_split < T_hi ? t_lo + per_split : T_hi;
  float m[CSC_CLASSES], l[CSC_CLASSES], rs = 0.f;
  int cnt[CSC_CLASSES];
#pragma unroll
  for (int c = 0; c < CSC_CLASSES; ++c) m[c] = -INFINITY, l[c] = 0.f, cnt[c] = 0;
  for (int64_t tile = t_lo; tile < t_hi; ++tile) {
    __syncthreads();
    nce_stage(B, tile * NCE_TILE, P, C, LDW, img);
    if (threadIdx.x < NCE_TILE) {
      const int64_t r = tile * NCE_TILE + threadIdx.x;
      float4 o;
      o.x = o.y = o.z = 0.f;
      o.w = __int_as_float(-1);
      if (r < P) o = xs1[r];
      xt[threadIdx.x] = o;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NCE_TILE / 16; ++t) {
      const f32x4 s = nce_scores<CH>(img, LDW, t, j, g, stat);
      float z[4], e[4], mt[CSC_CLASSES];
      int cl[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lc = 16 * t + 4 * g + r;
        const float4 o = xt[lc];
        const bool v = row_ok && __float_as_int(o.w) == my_scene;
        const bool dg = tile * NCE_TILE + lc == sr;
        cl[r] = v ? csc_class(o.x, o.y, o.z, me.x, me.y, me.z, r1, r2) : -1;
        z[r] = (v && !dg) ? nce_logit(s[r], inv_t) : -INFINITY;
        rs += v ? s[r] : 0.f;
        if (v && dg) diag[sr] = s[r];
      }
#pragma unroll
      for (int c = 0; c < CSC_CLASSES; ++c) {
        mt[c] = m[c];
#pragma unroll
        for (int r = 0; r < 4; ++r) mt[c] = fmaxf(mt[c], cl[r] == c ? z[r] : -INFINITY);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float ms = mt[0];
#pragma unroll
        for (int c = 1; c < CSC_CLASSES; ++c) ms = cl[r] == c ? mt[c] : ms;
        e[r] = z[r] == -INFINITY ? 0.f : __expf(z[r] - ms);
      }
#pragma unroll
      for (int c = 0; c < CSC_CLASSES; ++c) {
        float a = mt[c] == -INFINITY ? 0.f : l[c] * __expf(m[c] - mt[c]);      // m = -inf: l is 0 and exp(-inf) = 0
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          a += cl[r] == c ? e[r] : 0.f;
          cnt[c] += cl[r] == c ? 1 : 0;
        }
        l[c] = a;
        m[c] = mt[c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CSC_CLASSES; ++c) {
    csc_merge4(m[c], l[c], g);
    cnt[c] += __shfl_xor(cnt[c], 16, 64);
    cnt[c] += __shfl_xor(cnt[c], 32, 64);
  }
  const float r1s = __shfl_xor(rs, 16, 64);
  const float rp = (g & 1) ? r1s + rs : rs + r1s;
  const float r2s = __shfl_xor(rp, 32, 64);
  const float R = (g & 2) ? r2s + rp : rp + r2s;
  if (g == 0 && sr < P) {
    float* o = part + ((int64_t)blockIdx.y * P + sr) * CSC_PART;
#pragma unroll
    for (int c = 0; c < CSC_CLASSES; ++c) {
      o[c] = m[c];
      o[CSC_CLASSES + c] = l[c];
      reinterpret_cast<int32_t*>(o)[2 * CSC_CLASSES + c] = cnt[c];
    }
    o[3 * CSC_CLASSES] = R;
  }
}

// one workgroup per scene.  Merges the splits of each of its rows in order and adds the diagonal: lse[row][c] = log(exp(z_ii) + sum over
// the members of class c); a row without members gets z_ii itself, so its term is exactly 0.  The scene's member counts decide
// which classes are present (the diagonal included, as part.unique() sees it, :244); the lse of an absent class is then set to
// +inf.  For the backward the row's softmax keeps its two factors, rmax = the max (diagonal included) and rinv = 1 / the sum of
// exp(z - max): exp(z - rmax) * rinv has the error of torch's softmax, where exp(z - lse) would carry the rounding of an lse of
// size log(P_b) + 1 / t into every element of the row, all with one sign (a zero feature row multiplies that by 1 / 1e-7).
// rinv = 0 for an absent class.  roww = 1 / (nb partitions P_b).  Double accumulators, fixed tree.
// scene_out [nb][4]: sum over the present classes of mean_i(lse_c - z_ii), mean diagonal, mean of S, P_b.
__global__ void __launch_bounds__(MSC_THREADS)
csc_scene_kernel(const float* __restrict__ part, const float* __restrict__ diag, const int32_t* __restrict__ start, int64_t P, int n_split, int nb,
                 float inv_t, int partitions, float* __restrict__ lse, float* __restrict__ rmax, float* __restrict__ rinv, float* __restrict__ roww,
                 double* __restrict__ scene_out, int64_t* __restrict__ counts) {
  constexpr int NA = 2 * CSC_CLASSES + 2;
  __shared__ double red[NA][MSC_THREADS];
  const int b = blockIdx.x;
  const int64_t lo = start[b], hi = start[b + 1], n = hi - lo;
  double acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += MSC_THREADS) {
    const float zd = nce_logit(diag[i], inv_t);
#pragma unroll
    for (int c = 0; c < CSC_CLASSES; ++c) {
      float M = -INFINITY;
      for (int s = 0; s < n_split; ++s) M = fmaxf(M, part[((int64_t)s * P + i) * CSC_PART + c]);
      float L = 0.f;
      int64_t members = 0;
      for (int s = 0; s < n_split; ++s) {
        const float* p = part + ((int64_t)s * P + i) * CSC_PART;
        L += p[c] == -INFINITY ? 0.f : p[CSC_CLASSES + c] * __expf(p[c] - M);
        members += reinterpret_cast<const int32_t*>(p)[2 * CSC_CLASSES + c];
      }
      float v = zd, Mx = zd, Lx = 1.f;
      if (M != -INFINITY) {
        Mx = fmaxf(M, zd);
        Lx = L * __expf(M - Mx) + __expf(zd - Mx);
        v = Mx + __logf(Lx);
      }
      lse[i * CSC_CLASSES + c] = v;
      rmax[i * CSC_CLASSES + c] = Mx;
      rinv[i * CSC_CLASSES + c] = 1.0f / Lx;
      acc[c] += (double)(v - zd);
      acc[CSC_CLASSES + c] += (double)members;
    }
    float R = 0.f;
    for (int s = 0; s < n_split; ++s) R += part[((int64_t)s * P + i) * CSC_PART + 3 * CSC_CLASSES];
    acc[2 * CSC_CLASSES] += (double)diag[i];
    acc[2 * CSC_CLASSES + 1] += (double)(R / (float)n);
  }
#pragma unroll
  for (int a = 0; a < NA; ++a) red[a][threadIdx.x] = acc[a];
  __syncthreads();
  for (int o = MSC_THREADS / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int a = 0; a < NA; ++a) red[a][threadIdx.x] += red[a][threadIdx.x + o];
    __syncthreads();
  }
  bool present[CSC_CLASSES];
#pragma unroll
  for (int c = 0; c < CSC_CLASSES; ++c) present[c] = red[CSC_CLASSES + c][0] > 0.0;
  const float w = n > 0 ? 1.0f / ((float)nb * (float)partitions * (float)n) : 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += MSC_THREADS) {
#pragma unroll
    for (int c = 0; c < CSC_CLASSES; ++c)
      if (!present[c]) lse[i * CSC_CLASSES + c] = INFINITY, rinv[i * CSC_CLASSES + c] = 0.f;
    roww[i] = w;
  }
  if (threadIdx.x == 0) {
    double loss = 0.0;
#pragma unroll
    for (int c = 0; c < CSC_CLASSES; ++c) {
      if (present[c]) loss += red[c][0];
      counts[(int64_t)b * CSC_CLASSES + c] = (int64_t)red[CSC_CLASSES + c][0];
    }
    double* o = scene_out + (int64_t)b * 4;
    o[0] = n > 0 ? loss / (double)n : 0.0;
    o[1] = n > 0 ? red[2 * CSC_CLASSES][0] / (double)n : 0.0;
    o[2] = n > 0 ? red[2 * CSC_CLASSES + 1][0] / (double)n : 0.0;
    o[3] = (double)n;
  }
}

// the scenes in ascending order, with the reference's running sum (:237-238: pos_sim is added to before neg_sim reads it)
__global__ void csc_final_kernel(const double* __restrict__ scene_out, int nb, int partitions, float* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double loss = 0.0, run = 0.0, neg = 0.0;
  for (int b = 0; b < nb; ++b) {
    const double* o = scene_out + (int64_t)b * 4;
    if (!(o[3] > 0.0)) continue;
    loss += o[0];
    run += o[1];
    neg += o[2] - run / o[3];
  }
  out[0] = (float)(loss / ((double)nb * (double)partitions));
  out[1] = (float)(run / (double)nb);
  out[2] = (float)(neg / (double)nb);
}

// backward products, as nce_bwd_kernel: blockIdx.y = 0: stationary A rows i, dA = G B;  1: stationary B rows j, dB = G^T A, with
// G[i][j] = w_b p_c(i, j) off the diagonal, c = class(i, j), and w_b sum over present c of (p_c(i, i) - 1) on it, where
// p_c(i, j) = exp(z_ij - rmax[i][c]) rinv[i][c] (= exp(z_ij - lse[i][c]); 0 for an absent class),
// w_b = dloss roww / t.  i and j share a scene wherever G is not 0, so the stationary row's own roww serves both roles.
template <int CH>
__global__ void __launch_bounds__(MSC_THREADS)
csc_bwd_kernel(const float* __restrict__ A, const float* __restrict__ B, const float4* __restrict__ xs1, const float4* __restrict__ xs2,
               const int32_t* __restrict__ start, const float* __restrict__ rmax, const float* __restrict__ rinv,
               const float* __restrict__ roww, const float* __restrict__ dloss, int64_t P, int C, int nb, float inv_t, float r1, float r2, float* __restrict__ gA,
               float* __restrict__ gB) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* img = reinterpret_cast<float*>(smem);
  constexpr int LDW = 16 * CH + 4;
  float4* xt = reinterpret_cast<float4*>(img + NCE_TILE * LDW);
  float* max_t = img + NCE_TILE * LDW + NCE_TILE * 4;
  float* inv_t_ = max_t + NCE_TILE * CSC_CLASSES;
  const bool role_b = blockIdx.y != 0;
  const float* S_ = role_b ? B : A;          // stationary
  const float* T_ = role_b ? A : B;          // streamed
  const float4* xs_s = role_b ? xs1 : xs2;   // row i carries x2[i], column j carries x1[j]
  const float4* xs_t = role_b ? xs2 : xs1;
  float* out = role_b ? gB : gA;
  const int lane = ptc_lane(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int64_t sr = (int64_t)blockIdx.x * NCE_ROWS + wave * 16 + j;
  f32x4 stat[CH], acc[CH];
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    const int c = 16 * ch + 4 * g;
    stat[ch] = (sr < P && c < C) ? *reinterpret_cast<const f32x4*>(S_ + sr * C + c) : nce_splat(0.f);
    acc[ch] = nce_splat(0.f);
  }
  float4 me;
  me.x = me.y = me.z = 0.f;
  me.w = __int_as_float(nb);
  if (sr < P) me = xs_s[sr];
  const int my_scene = __float_as_int(me.w);
  const bool row_ok = sr < P && my_scene < nb;
  const float gs = row_ok ? dloss[0] * inv_t * roww[sr] : 0.f;
  float max_s[CSC_CLASSES], inv_s[CSC_CLASSES];
#pragma unroll
  for (int c = 0; c < CSC_CLASSES; ++c) {
    max_s[c] = (!role_b && row_ok) ? rmax[sr * CSC_CLASSES + c] : 0.f;
    inv_s[c] = (!role_b && row_ok) ? rinv[sr * CSC_CLASSES + c] : 0.f;
  }
  float ones = 0.f;                          // the -1s of the diagonal element, met by one of the row's four lanes
  int64_t t_lo, t_hi;
  csc_tile_range(xs_s, start, P, nb, t_lo, t_hi);
  for (int64_t tile = t_lo; tile < t_hi; ++tile) {
    __syncthreads();
    nce_stage(T_, tile * NCE_TILE, P, C, LDW, img);
    if (threadIdx.x < NCE_TILE) {
      const int64_t r = tile * NCE_TILE + threadIdx.x;
      float4 o;
      o.x = o.y = o.z = 0.f;
      o.w = __int_as_float(-1);
      if (r < P) o = xs_t[r];
      xt[threadIdx.x] = o;
    }
    for (int i = threadIdx.x; i < NCE_TILE * CSC_CLASSES; i += MSC_THREADS) {
      const int64_t r = tile * NCE_TILE + i / CSC_CLASSES;
      max_t[i] = (role_b && r < P) ? rmax[tile * NCE_TILE * CSC_CLASSES + i] : 0.f;
      inv_t_[i] = (role_b && r < P) ? rinv[tile * NCE_TILE * CSC_CLASSES + i] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NCE_TILE / 16; ++t) {
      const f32x4 s = nce_scores<CH>(img, LDW, t, j, g, stat);
      f32x4 w;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lc = 16 * t + 4 * g + r;
        const float4 o = xt[lc];
        const bool v = row_ok && __float_as_int(o.w) == my_scene;
        const int k = role_b ? csc_class(me.x, me.y, me.z, o.x, o.y, o.z, r1, r2) : csc_class(o.x, o.y, o.z, me.x, me.y, me.z, r1, r2);
        const float z = nce_logit(s[r], inv_t);
        float mx[CSC_CLASSES], iv[CSC_CLASSES];
#pragma unroll
        for (int c = 0; c < CSC_CLASSES; ++c) {
          mx[c] = role_b ? max_t[lc * CSC_CLASSES + c] : max_s[c];
          iv[c] = role_b ? inv_t_[lc * CSC_CLASSES + c] : inv_s[c];
        }
        float p;
        if (tile * NCE_TILE + lc == sr) {
          // the diagonal: sum over the present classes of (p_c - 1).  Only the p_c go through the accumulators; the -1s, several
          // times the size of everything else a row adds up, are taken off once at the end.  A class without members in this
          // row has p_c == 1 exactly and is left out of both.
          p = 0.f;
#pragma unroll
          for (int c = 0; c < CSC_CLASSES; ++c) {
            const float pc = __expf(z - mx[c]) * iv[c];
            const bool in = iv[c] > 0.f && pc != 1.f;
            p += in ? pc : 0.f;
            ones += (v && in) ? 1.f : 0.f;
          }
        } else {
          float mk = mx[0], ik = iv[0];
#pragma unroll
          for (int c = 1; c < CSC_CLASSES; ++c) mk = k == c ? mx[c] : mk, ik = k == c ? iv[c] : ik;
          p = __expf(z - mk) * ik;
        }
        w[r] = v ? p * gs : 0.f;
      }
      // acc[channels 16 ch + 4 g ..][row j] += sum over the 16 streamed rows: lane (c', k) reads column c' of rows 4 k + r
      const float* col = img + (16 * t + 4 * g) * LDW + j;
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) {
        acc[ch] = ptc_mfma_f32_4(col[16 * ch], w[0], acc[ch]);
        acc[ch] = ptc_mfma_f32_4(col[16 * ch + LDW], w[1], acc[ch]);
        acc[ch] = ptc_mfma_f32_4(col[16 * ch + 2 * LDW], w[2], acc[ch]);
        acc[ch] = ptc_mfma_f32_4(col[16 * ch + 3 * LDW], w[3], acc[ch]);
      }
    }
  }
  ones += __shfl_xor(ones, 16, 64);
  ones += __shfl_xor(ones, 32, 64);
  if (sr < P) {
    const float k = ones * gs;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
      const int c = 16 * ch + 4 * g;
      if (c < C) {
        const f32x4 partner = *reinterpret_cast<const f32x4*>(T_ + sr * C + c);       // row sr of the other side: B_i for dA_i, A_j for dB_j
        *reinterpret_cast<f32x4*>(out + sr * C + c) = acc[ch] - partner * k;
      }
    }
  }
}

namespace {

int nce_ch(int C) { return C <= 32 ? 2 : C <= 64 ? 4 : C <= 96 ? 6 : C <= 128 ? 8 : 16; }
int nce_split(int64_t P) {
  const int64_t blocks = ptc_cdiv(P, NCE_ROWS), tiles = ptc_cdiv(P, NCE_TILE);
  int64_t s = 512 / (blocks > 0 ? blocks : 1);
  s = s < 1 ? 1 : (s > NCE_MAX_SPLIT ? NCE_MAX_SPLIT : s);
  return (int)(s > tiles ? (tiles > 0 ? tiles : 1) : s);
}
size_t nce_lds(int ch) { return (size_t)(NCE_TILE * (16 * ch + 4) + NCE_TILE) * 4; }

struct NceLayout {
  size_t part, diag, ga, gb, keys, order, skeys, scratch, total;
};
NceLayout nce_layout(int64_t P, int C) {
  NceLayout Y;
  PtcArena A;
  const int64_t p = P > 0 ? P : 1;
  Y.part = A.take((size_t)p * 3 * 4 * NCE_MAX_SPLIT);
  Y.diag = A.take((size_t)p * 4);
  Y.ga = A.take((size_t)p * C * 4);
  Y.gb = A.take((size_t)p * C * 4);
  Y.keys = A.take((size_t)p * 8);
  Y.order = A.take((size_t)p * 8);
  Y.skeys = A.take((size_t)p * 8);
  Y.scratch = A.take(ptc_sort_keys_workspace_bytes(p, 1));
  Y.total = A.total;
  return Y;
}

int nce_check(int64_t P, int C) {
  PTC_REQUIRE(P >= 1, PTC_EINVAL, "ptc_msc_nce: P=%lld (needs at least one matched pair)", (long long)P);
  PTC_REQUIRE(P <= NCE_MAX_P, PTC_EUNSUPPORTED, "ptc_msc_nce: P=%lld above %d pairs", (long long)P, NCE_MAX_P);
  PTC_REQUIRE(C >= 4 && C <= 256 && (C & 3) == 0, PTC_EUNSUPPORTED, "ptc_msc_nce: C=%d is not a multiple of 4 in [4, 256]", C);
  return PTC_OK;
}

size_t csc_lds(int ch) { return (size_t)(NCE_TILE * (16 * ch + 4) + NCE_TILE * 4 + 2 * NCE_TILE * CSC_CLASSES) * 4; }

// `big` holds the forward's split partials or the backward's two gradient images, never both
struct CscLayout {
  size_t big, diag, scene_out, keys, order, skeys, scratch, total;
};
CscLayout csc_layout(int64_t P, int C, int nb) {
  CscLayout Y;
  PtcArena A;
  const int64_t p = P > 0 ? P : 1;
  const size_t part = (size_t)p * CSC_PART * 4 * NCE_MAX_SPLIT, grads = 2 * ptc_align_up((size_t)p * C * 4, 256);
  Y.big = A.take(part > grads ? part : grads);
  Y.diag = A.take((size_t)p * 4);
  Y.scene_out = A.take((size_t)(nb > 0 ? nb : 1) * 4 * 8);
  Y.keys = A.take((size_t)p * 8);
  Y.order = A.take((size_t)p * 8);
  Y.skeys = A.take((size_t)p * 8);
  Y.scratch = A.take(ptc_sort_keys_workspace_bytes(p, 1));
  Y.total = A.total;
  return Y;
}

int csc_check(int64_t P, int C, int nb, float nce_t, float r1, float r2, int partitions) {
  int rc = nce_check(P, C);
  if (rc != PTC_OK) return rc;
  PTC_REQUIRE(nb >= 1 && nb <= CSC_MAX_SCENES, PTC_EINVAL, "ptc_msc_csc_nce: %d scenes not in [1, %d]", nb, CSC_MAX_SCENES);
  PTC_REQUIRE(nce_t > 0.f && partitions >= 1, PTC_EINVAL, "ptc_msc_csc_nce: nce_t and partitions must be positive");
  PTC_REQUIRE(r1 <= r2, PTC_EINVAL, "ptc_msc_csc_nce: needs r1 <= r2, got r1=%g r2=%g", (double)r1, (double)r2);
  return PTC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t ptc_msc_match_workspace_bytes(int64_t n) { return match_layout(n).total; }

extern "C" int ptc_msc_match(const float* xyz, const int32_t* offset, const float* new_xyz, const int32_t* new_offset, int b, int64_t n,
                             int64_t m, int k, float max_radius, int32_t* count, int32_t* cand, int32_t* stats, void* workspace,
                             size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && m >= 0 && b >= 1 && b < 32767, PTC_EINVAL, "ptc_msc_match: bad sizes");
  PTC_REQUIRE(k >= 1 && k <= MSC_KMAX, PTC_EUNSUPPORTED, "ptc_msc_match: k=%d not in [1,%d]", k, MSC_KMAX);
  PTC_REQUIRE(n < (1ll << 31) && m * k < (1ll << 40), PTC_EUNSUPPORTED, "ptc_msc_match: too many points");
  PTC_REQUIRE(max_radius == max_radius && max_radius < INFINITY, PTC_EINVAL, "ptc_msc_match: max_radius must be finite");
  PTC_REQUIRE(stats, PTC_EINVAL, "ptc_msc_match: null stats");
  const MatchLayout Y = match_layout(n);
  PTC_REQUIRE(workspace && workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_msc_match: workspace %zu < %zu", workspace_bytes, Y.total);
  PTC_REQUIRE(m == 0 || (count && cand && new_xyz && new_offset), PTC_EINVAL, "ptc_msc_match: null buffer");
  hipStream_t s = (hipStream_t)stream;
  if (m == 0 || n == 0 || !(max_radius > 0.f)) {
    hipLaunchKernelGGL(msc_zero_match_kernel, dim3(msc_grid1(m * k)), dim3(MSC_THREADS), 0, s, m, k, count, cand, stats);
    PTC_CHECK_LAUNCH("msc_zero_match_kernel");
    return PTC_OK;
  }
  PTC_REQUIRE(xyz && offset, PTC_EINVAL, "ptc_msc_match: null buffer");
  char* ws = (char*)workspace;
  PtcCellGrid* grid = (PtcCellGrid*)(ws + Y.g.grid);
  int64_t* keys = (int64_t*)(ws + Y.g.keys);
  int64_t* skeys = (int64_t*)(ws + Y.g.skeys);
  float4* sxyz = (float4*)(ws + Y.g.sxyz);
  int rc = ptc_cell_grid_params(xyz, n, (double)max_radius, (uint32_t*)(ws + Y.g.mm), grid, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(msc_keys_kernel, dim3(msc_grid1(n)), dim3(MSC_THREADS), 0, s, xyz, offset, b, n, grid, keys, stats);
  PTC_CHECK_LAUNCH("msc_keys_kernel");
  int scene_bits = 1;
  while ((1 << scene_bits) <= b) ++scene_bits;
  rc = ptc_cell_grid_sort(xyz, keys, n, 48 + scene_bits, (int64_t*)(ws + Y.g.order), skeys, sxyz, ws + Y.g.scratch, Y.g.scratch_bytes, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(msc_match_kernel, dim3(msc_grid1(m)), dim3(MSC_THREADS), 0, s, new_xyz, new_offset, b, m, grid, skeys, sxyz, n, k,
                     max_radius, count, cand, stats);
  PTC_CHECK_LAUNCH("msc_match_kernel");
  return PTC_OK;
}

extern "C" size_t ptc_msc_select_workspace_bytes(int64_t m) {
  const int64_t c = m > 0 ? m : 1;
  return ptc_align_up((size_t)c * 4, 256) + ptc_align_up((size_t)c * 8, 256) + ptc_exclusive_scan_workspace_bytes(c);
}

extern "C" int ptc_msc_select(const int32_t* count, const int32_t* cand, int64_t m, int k, const int64_t* r, int64_t n_matched,
                              int64_t* match_index, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(m >= 0 && n_matched >= 0 && n_matched <= m, PTC_EINVAL, "ptc_msc_select: bad sizes");
  PTC_REQUIRE(k >= 1 && k <= MSC_KMAX, PTC_EUNSUPPORTED, "ptc_msc_select: k=%d not in [1,%d]", k, MSC_KMAX);
  if (m == 0 || n_matched == 0) return PTC_OK;
  PTC_REQUIRE(count && cand && r && match_index, PTC_EINVAL, "ptc_msc_select: null buffer");
  PTC_REQUIRE(workspace && workspace_bytes >= ptc_msc_select_workspace_bytes(m), PTC_EWORKSPACE, "ptc_msc_select: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* flag = (int32_t*)ws;
  int64_t* rank = (int64_t*)(ws + ptc_align_up((size_t)m * 4, 256));
  char* scan_ws = (char*)rank + ptc_align_up((size_t)m * 8, 256);
  hipLaunchKernelGGL(msc_flags_kernel, dim3(msc_grid1(m)), dim3(MSC_THREADS), 0, s, count, m, flag);
  PTC_CHECK_LAUNCH("msc_flags_kernel");
  int rc = ptc_exclusive_scan_i32(flag, m, rank, scan_ws, ptc_exclusive_scan_workspace_bytes(m), stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(msc_select_kernel, dim3(msc_grid1(m)), dim3(MSC_THREADS), 0, s, count, cand, rank, m, k, r, n_matched, match_index);
  PTC_CHECK_LAUNCH("msc_select_kernel");
  return PTC_OK;
}

extern "C" size_t ptc_msc_patch_workspace_bytes(int64_t n_total) { return patch_layout(n_total).total; }

extern "C" int ptc_msc_patch_rank(const float* cell1, const int32_t* offset1, int64_t n1, const float* cell2, const int32_t* offset2,
                                  int64_t n2, int b, int32_t* cluster, int64_t* patch_num, void* workspace, size_t workspace_bytes,
                                  ptc_stream_t stream) {
  PTC_REQUIRE(n1 >= 0 && n2 >= 0 && b >= 1 && n1 + n2 < (1ll << 31), PTC_EINVAL, "ptc_msc_patch_rank: bad sizes");
  PTC_REQUIRE(patch_num, PTC_EINVAL, "ptc_msc_patch_rank: null patch_num");
  const int64_t n = n1 + n2;
  hipStream_t s = (hipStream_t)stream;
  PTC_HIP(hipMemsetAsync(patch_num, 0, 8, s));
  if (n == 0) return PTC_OK;
  PTC_REQUIRE(cluster && offset1 && offset2 && (n1 == 0 || cell1) && (n2 == 0 || cell2), PTC_EINVAL, "ptc_msc_patch_rank: null buffer");
  const PatchLayout Y = patch_layout(n);
  PTC_REQUIRE(workspace && workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_msc_patch_rank: workspace %zu < %zu", workspace_bytes, Y.total);
  char* ws = (char*)workspace;
  uint32_t* mx = (uint32_t*)(ws + Y.mx);
  int64_t* keys = (int64_t*)(ws + Y.keys);
  int64_t* order = (int64_t*)(ws + Y.order);
  int64_t* skeys = (int64_t*)(ws + Y.skeys);
  int32_t* flag = (int32_t*)(ws + Y.flag);
  int64_t* scan = (int64_t*)(ws + Y.scan);
  PTC_HIP(hipMemsetAsync(mx, 0, 12, s));
  int gb = msc_grid1(n);
  gb = gb > 1024 ? 1024 : gb;
  hipLaunchKernelGGL(msc_cell_max_kernel, dim3(gb), dim3(MSC_THREADS), 0, s, cell1, n1, cell2, n2, mx);
  PTC_CHECK_LAUNCH("msc_cell_max_kernel");
  hipLaunchKernelGGL(msc_patch_ids_kernel, dim3(msc_grid1(n)), dim3(MSC_THREADS), 0, s, cell1, offset1, n1, cell2, offset2, n2, b, mx, keys);
  PTC_CHECK_LAUNCH("msc_patch_ids_kernel");
  int rc = ptc_sort_keys_ex(keys, n, 1, 0, 64, order, nullptr, skeys, ws + Y.scratch, Y.total - Y.scratch, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(msc_run_flags_kernel, dim3(msc_grid1(n)), dim3(MSC_THREADS), 0, s, skeys, n, flag);
  PTC_CHECK_LAUNCH("msc_run_flags_kernel");
  rc = ptc_exclusive_scan_i32(flag, n, scan, ws + Y.scratch, Y.total - Y.scratch, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(msc_ranks_kernel, dim3(msc_grid1(n)), dim3(MSC_THREADS), 0, s, flag, scan, order, n, cluster, patch_num);
  PTC_CHECK_LAUNCH("msc_ranks_kernel");
  return PTC_OK;
}

extern "C" int ptc_msc_patch_masks(const int32_t* cluster, const int32_t* patch_mask, int64_t patch_num, int64_t n1, int64_t n2,
                                   uint8_t* mask1, uint8_t* mask2, ptc_stream_t stream) {
  PTC_REQUIRE(n1 >= 0 && n2 >= 0 && patch_num >= 0, PTC_EINVAL, "ptc_msc_patch_masks: bad sizes");
  if (n1 + n2 == 0) return PTC_OK;
  PTC_REQUIRE(cluster && (patch_num == 0 || patch_mask) && (n1 == 0 || mask1) && (n2 == 0 || mask2), PTC_EINVAL,
              "ptc_msc_patch_masks: null buffer");
  hipLaunchKernelGGL(msc_patch_masks_kernel, dim3(msc_grid1(n1 + n2)), dim3(MSC_THREADS), 0, (hipStream_t)stream, cluster, patch_mask,
                     patch_num, n1, n2, mask1, mask2);
  PTC_CHECK_LAUNCH("msc_patch_masks_kernel");
  return PTC_OK;
}

extern "C" size_t ptc_msc_nce_workspace_bytes(int64_t p, int c) { return nce_layout(p, c).total; }

extern "C" int ptc_msc_nce_fwd(const float* feat1, int64_t n1, const float* feat2, int64_t n2, const int64_t* match_index, int64_t p, int c,
                               float nce_t, float* an, float* bn, float* na, float* nb, float* lse, float* out, void* workspace,
                               size_t workspace_bytes, ptc_stream_t stream) {
  int rc = nce_check(p, c);
  if (rc != PTC_OK) return rc;
  PTC_REQUIRE(nce_t > 0.f && n1 >= 0 && n2 >= 0, PTC_EINVAL, "ptc_msc_nce_fwd: bad nce_t / sizes");
  PTC_REQUIRE(match_index && an && bn && na && nb && lse && out && (n1 == 0 || feat1) && (n2 == 0 || feat2), PTC_EINVAL,
              "ptc_msc_nce_fwd: null buffer");
  const NceLayout Y = nce_layout(p, c);
  PTC_REQUIRE(workspace && workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_msc_nce_fwd: workspace %zu < %zu", workspace_bytes, Y.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* part = (float*)(ws + Y.part);
  float* diag = (float*)(ws + Y.diag);
  const unsigned rows4 = (unsigned)ptc_cdiv(p, MSC_THREADS / 64);
  hipLaunchKernelGGL(nce_gather_norm_kernel, dim3(rows4), dim3(MSC_THREADS), 0, s, feat1, n1, match_index, 0, p, c, an, na);
  PTC_CHECK_LAUNCH("nce_gather_norm_kernel");
  hipLaunchKernelGGL(nce_gather_norm_kernel, dim3(rows4), dim3(MSC_THREADS), 0, s, feat2, n2, match_index, 1, p, c, bn, nb);
  PTC_CHECK_LAUNCH("nce_gather_norm_kernel");
  const int ch = nce_ch(c), n_split = nce_split(p);
  const int tiles_per_split = (int)ptc_cdiv(ptc_cdiv(p, NCE_TILE), n_split);
  const size_t lds = nce_lds(ch);
  const dim3 grid((unsigned)ptc_cdiv(p, NCE_ROWS), (unsigned)n_split);
  const float inv_t = 1.0f / nce_t;
#define NCE_FWD(CH)                                                                                                       \
  do {                                                                                                                    \
    rc = ptc_allow_lds(nce_fwd_kernel<CH>, lds);                                                                          \
    if (rc != PTC_OK) return rc;                                                                                          \
    hipLaunchKernelGGL(nce_fwd_kernel<CH>, grid, dim3(MSC_THREADS), lds, s, an, bn, p, c, inv_t, tiles_per_split, part, diag); \
  } while (0)
  switch (ch) {
    case 2: NCE_FWD(2); break;
    case 4: NCE_FWD(4); break;
    case 6: NCE_FWD(6); break;
    case 8: NCE_FWD(8); break;
    default: NCE_FWD(16); break;
  }
#undef NCE_FWD
  PTC_CHECK_LAUNCH("nce_fwd_kernel");
  hipLaunchKernelGGL(nce_finish_kernel, dim3(1), dim3(MSC_THREADS), 0, s, part, diag, p, n_split, inv_t, lse, out);
  PTC_CHECK_LAUNCH("nce_finish_kernel");
  return PTC_OK;
}

extern "C" int ptc_msc_nce_bwd(const float* an, const float* bn, const float* na, const float* nb, const float* lse,
                               const int64_t* match_index, int64_t p, int c, int64_t n1, int64_t n2, float nce_t, const float* dloss,
                               float* dfeat1, float* dfeat2, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  int rc = nce_check(p, c);
  if (rc != PTC_OK) return rc;
  PTC_REQUIRE(nce_t > 0.f && n1 >= 0 && n2 >= 0, PTC_EINVAL, "ptc_msc_nce_bwd: bad nce_t / sizes");
  PTC_REQUIRE(an && bn && na && nb && lse && match_index && dloss && (n1 == 0 || dfeat1) && (n2 == 0 || dfeat2), PTC_EINVAL,
              "ptc_msc_nce_bwd: null buffer");
  const NceLayout Y = nce_layout(p, c);
  PTC_REQUIRE(workspace && workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_msc_nce_bwd: workspace %zu < %zu", workspace_bytes, Y.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* ga = (float*)(ws + Y.ga);
  float* gb = (float*)(ws + Y.gb);
  int64_t* keys = (int64_t*)(ws + Y.keys);
  int64_t* order = (int64_t*)(ws + Y.order);
  int64_t* skeys = (int64_t*)(ws + Y.skeys);
  const int ch = nce_ch(c);
  const size_t lds = nce_lds(ch);
  const dim3 grid((unsigned)ptc_cdiv(p, NCE_ROWS), 2);
  const float inv_t = 1.0f / nce_t;
#define NCE_BWD(CH)                                                                                                 \
  do {                                                                                                              \
    rc = ptc_allow_lds(nce_bwd_kernel<CH>, lds);                                                                    \
    if (rc != PTC_OK) return rc;                                                                                    \
    hipLaunchKernelGGL(nce_bwd_kernel<CH>, grid, dim3(MSC_THREADS), lds, s, an, bn, lse, dloss, p, c, inv_t, ga, gb); \
  } while (0)
  switch (ch) {
    case 2: NCE_BWD(2); break;
    case 4: NCE_BWD(4); break;
    case 6: NCE_BWD(6); break;
    case 8: NCE_BWD(8); break;
    default: NCE_BWD(16); break;
  }
#undef NCE_BWD
  PTC_CHECK_LAUNCH("nce_bwd_kernel");
  const unsigned rows4 = (unsigned)ptc_cdiv(p, MSC_THREADS / 64);
  for (int side = 0; side < 2; ++side) {
    float* g = side ? gb : ga;
    const int64_t n_rows = side ? n2 : n1;
    float* dfeat = side ? dfeat2 : dfeat1;
    hipLaunchKernelGGL(nce_norm_bwd_kernel, dim3(rows4), dim3(MSC_THREADS), 0, s, side ? bn : an, side ? nb : na, p, c, g);
    PTC_CHECK_LAUNCH("nce_norm_bwd_kernel");
    if (n_rows == 0) continue;
    hipLaunchKernelGGL(nce_row_keys_kernel, dim3(msc_grid1(p)), dim3(MSC_THREADS), 0, s, match_index, side, p, n_rows, keys);
    PTC_CHECK_LAUNCH("nce_row_keys_kernel");
    int bits = 1;
    while (((int64_t)1 << bits) <= n_rows) ++bits;
    rc = ptc_sort_keys_ex(keys, p, 1, 0, bits, order, nullptr, skeys, ws + Y.scratch, Y.total - Y.scratch, stream);
    if (rc != PTC_OK) return rc;
    hipLaunchKernelGGL(nce_segment_add_kernel, dim3(msc_grid1(p * (c >> 2))), dim3(MSC_THREADS), 0, s, skeys, order, g, p, c, n_rows, dfeat);
    PTC_CHECK_LAUNCH("nce_segment_add_kernel");
  }
  return PTC_OK;
}

extern "C" size_t ptc_msc_csc_nce_workspace_bytes(int64_t p, int c, int nb) { return csc_layout(p, c, nb).total; }

extern "C" int ptc_msc_csc_nce_fwd(const float* feat1, int64_t n1, const float* feat2, int64_t n2, const float* coord1, const float* coord2,
                                   const int32_t* offset1, int nb, const int64_t* match_index, int64_t p, int c, float nce_t, float r1,
                                   float r2, int partitions, float* an, float* bn, float* na, float* nbn, float* xs1, float* xs2,
                                   int64_t* smatch, int32_t* start, float* lse, float* rmax, float* rinv, float* roww, int64_t* counts,
                                   float* out, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  int rc = csc_check(p, c, nb, nce_t, r1, r2, partitions);
  if (rc != PTC_OK) return rc;
  PTC_REQUIRE(n1 >= 0 && n2 >= 0, PTC_EINVAL, "ptc_msc_csc_nce_fwd: bad sizes");
  PTC_REQUIRE(match_index && offset1 && an && bn && na && nbn && xs1 && xs2 && smatch && start && lse && rmax && rinv && roww && counts && out &&
                  (n1 == 0 || (feat1 && coord1)) && (n2 == 0 || (feat2 && coord2)),
              PTC_EINVAL, "ptc_msc_csc_nce_fwd: null buffer");
  const CscLayout Y = csc_layout(p, c, nb);
  PTC_REQUIRE(workspace && workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_msc_csc_nce_fwd: workspace %zu < %zu", workspace_bytes, Y.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* part = (float*)(ws + Y.big);
  float* diag = (float*)(ws + Y.diag);
  double* scene_out = (double*)(ws + Y.scene_out);
  int64_t* keys = (int64_t*)(ws + Y.keys);
  int64_t* order = (int64_t*)(ws + Y.order);
  int64_t* skeys = (int64_t*)(ws + Y.skeys);
  hipLaunchKernelGGL(csc_scene_keys_kernel, dim3(msc_grid1(p)), dim3(MSC_THREADS), 0, s, match_index, p, n1, n2, offset1, nb, keys);
  PTC_CHECK_LAUNCH("csc_scene_keys_kernel");
  int bits = 1;
  while ((1 << bits) <= nb) ++bits;
  rc = ptc_sort_keys_ex(keys, p, 1, 0, bits, order, nullptr, skeys, ws + Y.scratch, Y.total - Y.scratch, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(csc_group_kernel, dim3(msc_grid1(p)), dim3(MSC_THREADS), 0, s, match_index, order, skeys, p, coord1, coord2, nb, smatch,
                     (float4*)xs1, (float4*)xs2, start);
  PTC_CHECK_LAUNCH("csc_group_kernel");
  const unsigned rows4 = (unsigned)ptc_cdiv(p, MSC_THREADS / 64);
  hipLaunchKernelGGL(nce_gather_norm_kernel, dim3(rows4), dim3(MSC_THREADS), 0, s, feat1, n1, smatch, 0, p, c, an, na);
  PTC_CHECK_LAUNCH("nce_gather_norm_kernel");
  hipLaunchKernelGGL(nce_gather_norm_kernel, dim3(rows4), dim3(MSC_THREADS), 0, s, feat2, n2, smatch, 1, p, c, bn, nbn);
  PTC_CHECK_LAUNCH("nce_gather_norm_kernel");
  const int ch = nce_ch(c), n_split = nce_split(p);
  const size_t lds = csc_lds(ch);
  const dim3 grid((unsigned)ptc_cdiv(p, NCE_ROWS), (unsigned)n_split);
  const float inv_t = 1.0f / nce_t;
#define CSC_FWD(CH)                                                                                                              \
  do {                                                                                                                           \
    rc = ptc_allow_lds(csc_fwd_kernel<CH>, lds);                                                                                 \
    if (rc != PTC_OK) return rc;                                                                                                 \
    hipLaunchKernelGGL(csc_fwd_kernel<CH>, grid, dim3(MSC_THREADS), lds, s, an, bn, (const float4*)xs1, (const float4*)xs2, start, p, c, nb, \
                       inv_t, r1, r2, part, diag);                                                                               \
  } while (0)
  switch (ch) {
    case 2: CSC_FWD(2); break;
    case 4: CSC_FWD(4); break;
    case 6: CSC_FWD(6); break;
    case 8: CSC_FWD(8); break;
    default: CSC_FWD(16); break;
  }
#undef CSC_FWD
  PTC_CHECK_LAUNCH("csc_fwd_kernel");
  hipLaunchKernelGGL(csc_scene_kernel, dim3(nb), dim3(MSC_THREADS), 0, s, part, diag, start, p, n_split, nb, inv_t, partitions, lse, rmax, rinv,
                     roww, scene_out, counts);
  PTC_CHECK_LAUNCH("csc_scene_kernel");
  hipLaunchKernelGGL(csc_final_kernel, dim3(1), dim3(64), 0, s, scene_out, nb, partitions, out);
  PTC_CHECK_LAUNCH("csc_final_kernel");
  return PTC_OK;
}

extern "C" int ptc_msc_csc_nce_bwd(const float* an, const float* bn, const float* na, const float* nbn, const float* xs1, const float* xs2,
                                   const int64_t* smatch, const int32_t* start, const float* rmax, const float* rinv, const float* roww,
                                   int64_t p, int c, int nb, int64_t n1, int64_t n2, float nce_t, float r1, float r2, const float* dloss, float* dfeat1,
                                   float* dfeat2, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  int rc = csc_check(p, c, nb, nce_t, r1, r2, 1);
  if (rc != PTC_OK) return rc;
  PTC_REQUIRE(n1 >= 0 && n2 >= 0, PTC_EINVAL, "ptc_msc_csc_nce_bwd: bad sizes");
  PTC_REQUIRE(an && bn && na && nbn && xs1 && xs2 && smatch && start && rmax && rinv && roww && dloss && (n1 == 0 || dfeat1) && (n2 == 0 || dfeat2),
              PTC_EINVAL, "ptc_msc_csc_nce_bwd: null buffer");
  const CscLayout Y = csc_layout(p, c, nb);
  PTC_REQUIRE(workspace && workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_msc_csc_nce_bwd: workspace %zu < %zu", workspace_bytes, Y.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* ga = (float*)(ws + Y.big);
  float* gb = (float*)(ws + Y.big + ptc_align_up((size_t)p * c * 4, 256));
  int64_t* keys = (int64_t*)(ws + Y.keys);
  int64_t* order = (int64_t*)(ws + Y.order);
  int64_t* skeys = (int64_t*)(ws + Y.skeys);
  const int ch = nce_ch(c);
  const size_t lds = csc_lds(ch);
  const dim3 grid((unsigned)ptc_cdiv(p, NCE_ROWS), 2);
  const float inv_t = 1.0f / nce_t;
#define CSC_BWD(CH)                                                                                                               \
  do {                                                                                                                            \
    rc = ptc_allow_lds(csc_bwd_kernel<CH>, lds);                                                                                  \
    if (rc != PTC_OK) return rc;                                                                                                  \
    hipLaunchKernelGGL(csc_bwd_kernel<CH>, grid, dim3(MSC_THREADS), lds, s, an, bn, (const float4*)xs1, (const float4*)xs2, start, rmax, rinv, \
                       roww, dloss, p, c, nb, inv_t, r1, r2, ga, gb);                                                                   \
  } while (0)
  switch (ch) {
    case 2: CSC_BWD(2); break;
    case 4: CSC_BWD(4); break;
    case 6: CSC_BWD(6); break;
    case 8: CSC_BWD(8); break;
    default: CSC_BWD(16); break;
  }
#undef CSC_BWD
  PTC_CHECK_LAUNCH("csc_bwd_kernel");
  const unsigned rows4 = (unsigned)ptc_cdiv(p, MSC_THREADS / 64);
  for (int side = 0; side < 2; ++side) {
    float* g = side ? gb : ga;
    const int64_t n_rows = side ? n2 : n1;
    float* dfeat = side ? dfeat2 : dfeat1;
    hipLaunchKernelGGL(nce_norm_bwd_kernel, dim3(rows4), dim3(MSC_THREADS), 0, s, side ? bn : an, side ? nbn : na, p, c, g);
    PTC_CHECK_LAUNCH("nce_norm_bwd_kernel");
    if (n_rows == 0) continue;
    hipLaunchKernelGGL(nce_row_keys_kernel, dim3(msc_grid1(p)), dim3(MSC_THREADS), 0, s, smatch, side, p, n_rows, keys);
    PTC_CHECK_LAUNCH("nce_row_keys_kernel");
    int bits = 1;
    while (((int64_t)1 << bits) <= n_rows) ++bits;
    rc = ptc_sort_keys_ex(keys, p, 1, 0, bits, order, nullptr, skeys, ws + Y.scratch, Y.total - Y.scratch, stream);
    if (rc != PTC_OK) return rc;
    hipLaunchKernelGGL(nce_segment_add_kernel, dim3(msc_grid1(p * (c >> 2))), dim3(MSC_THREADS), 0, s, skeys, order, g, p, c, n_rows, dfeat);
    PTC_CHECK_LAUNCH("nce_segment_add_kernel");
  }
  return PTC_OK;
}
