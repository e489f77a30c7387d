// pg_cluster.hip -- PointGroup's clustering (libs/pointgroup_ops: bfs_cluster_kernel.cu:16-61, bfs_cluster.cpp:53-145) and the fused
// heads' reductions of pointcept/models/point_group/point_group_v1m1_base.py:72-91,101-179.
//
// 1  Ball query.  Point k is a neighbour of query i iff both carry the same batch index and the fp32 expression
//    d2 = (ox-x)*(ox-x) + (oy-y)*(oy-y) + (oz-z)*(oz-z) (unfused, in that order) is < radius*radius; the list holds the first 1000
//    neighbours in ascending index order (the reference breaks at the 1001st).  A uniform grid of cells of edge >= |radius| (grown when
//    the extent would overflow the 16-bit cell fields of the packed key; cell_grid.h) is sorted with ptc_sort_keys, so each cell's points
//    are ascending by index.  The count pass counts hits over the 27 neighbour cells and stops at the 1001st (len = min(count, 1000)); an
//    exclusive scan gives exact starts, then the fill pass merges the 27 ascending cell lists and stops after `len` hits.  No per-thread
//    list buffer, no retry, no float atomics.  A point with a non-finite coordinate has no neighbour, not even itself.
// 2  Clustering.  Edges i->j for j in list(i) with label[j] == label[i].  Undirected components by a lock-free integer union-find
//    (CAS hooking of the larger root under the smaller, pointer jumping), so every representative is its component's minimum index.
//    Without a truncated list (len >= 1000 is taken as possibly truncated) the edges are symmetric and a component is exactly one
//    sequential-BFS cluster seeded at its minimum.  Any other component is resolved by the sequential rule itself, one workgroup per
//    component: ascending seeds, a level-synchronous frontier, visited flags in global memory.  A seed none of whose same-label
//    neighbours is larger than itself is a singleton (every smaller member is visited by then), which the workgroup takes a chunk at
//    a time.  Clusters below `threshold` are dropped (their points stay visited), the rest numbered in seed order; members are listed
//    in ascending point order.
// 3  Proposal scores: per cluster the member count, the class label[seed] and the mean of softmax(logits)[member, class], one
//    workgroup per cluster with a fixed-order reduction.  Dense [P, N] int32 proposal masks.
// 4  Bias losses (masked L1 + negative cosine) forward as two fixed-order reduction levels, and their backward in one pass.
#include "cell_grid.h"

#define PG_MAX_NBR PTC_PG_MAX_NEIGHBOURS
#define PG_THREADS 256
#define PG_SENTINEL 0x7fffffffffffffffll

namespace {

// the reference's expression, kept unfused
__device__ __forceinline__ bool pg_hit(float ox, float oy, float oz, float x, float y, float z, float r2) {
  return ptc_dist2(ox, oy, oz, x, y, z) < r2;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 1. ball query
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void pg_keys_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ bidx, int64_t n, int n_batch,
                               const PtcCellGrid* __restrict__ g, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
  const int b = bidx[i];
  if (!ptc_finite3(x, y, z) || b < 0 || b >= n_batch) {
    keys[i] = PG_SENTINEL;
    return;
  }
  const double e = g->edge;
  keys[i] = ptc_cell_key(b, ptc_cell(x, g->mn[0], e), ptc_cell(y, g->mn[1], e), ptc_cell(z, g->mn[2], e));
}

// the up to 27 non-empty sorted ranges [beg, end) of the cells around query i; returns their number
__device__ __forceinline__ int pg_ranges(const int64_t* __restrict__ skeys, int64_t n, int64_t key, int (&beg)[27], int (&end)[27]) {
  const int b = (int)(key >> 48), cz = (int)((key >> 32) & 0xffff), cy = (int)((key >> 16) & 0xffff), cx = (int)(key & 0xffff);
  int nl = 0;
  ptc_cell_runs(skeys, n, b, cx, cy, cz, [&](int64_t lo, int64_t hi, int y, int z) {      // each run split into its cells
    int64_t s = lo;
    for (int x = cx > 0 ? cx - 1 : 0; x <= cx + 1; ++x) {
      const int64_t e = x == cx + 1 ? hi : ptc_lower_bound(skeys, s, hi, ptc_cell_key(b, x + 1, y, z));
      if (e > s) {
        beg[nl] = (int)s;
        end[nl] = (int)e;
        ++nl;
      }
      s = e;
    }
  });
  return nl;
}

__global__ void __launch_bounds__(PG_THREADS) pg_count_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ keys,
                                                              const int64_t* __restrict__ skeys, const float4* __restrict__ sxyz,
                                                              int64_t n, float r2, int32_t* __restrict__ len, int32_t* __restrict__ trunc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t key = keys[i];
  int cnt = 0;
  if (key != PG_SENTINEL) {
    int beg[27], end[27];
    const int nl = pg_ranges(skeys, n, key, beg, end);
    const float ox = xyz[i * 3], oy = xyz[i * 3 + 1], oz = xyz[i * 3 + 2];
    for (int l = 0; l < nl && cnt <= PG_MAX_NBR; ++l)
      for (int p = beg[l]; p < end[l]; ++p) {
        const float4 q = sxyz[p];
        if (pg_hit(ox, oy, oz, q.x, q.y, q.z, r2) && ++cnt > PG_MAX_NBR) break;
      }
  }
  len[i] = cnt > PG_MAX_NBR ? PG_MAX_NBR : cnt;
  trunc[i] = cnt > PG_MAX_NBR ? 1 : 0;
}

__global__ void pg_start_len_kernel(const int32_t* __restrict__ len, const int32_t* __restrict__ trunc, const int64_t* __restrict__ start,
                                    int64_t n, int32_t* __restrict__ start_len, int64_t* __restrict__ total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  start_len[i * 2] = (int32_t)start[i];
  start_len[i * 2 + 1] = len[i];
  if (trunc[i]) atomicAdd((unsigned long long*)(total + 1), 1ull);
  if (i == n - 1) total[0] = start[i] + len[i];
}

__global__ void __launch_bounds__(PG_THREADS) pg_fill_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ keys,
                                                             const int64_t* __restrict__ skeys, const float4* __restrict__ sxyz,
                                                             int64_t n, float r2, const int32_t* __restrict__ start_len,
                                                             int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int want = start_len[i * 2 + 1];
  if (want == 0) return;
  int32_t* out = idx + start_len[i * 2];
  int beg[27], end[27], head[27];
  int nl = pg_ranges(skeys, n, keys[i], beg, end);
  for (int l = 0; l < nl; ++l) head[l] = __float_as_int(sxyz[beg[l]].w);
  const float ox = xyz[i * 3], oy = xyz[i * 3 + 1], oz = xyz[i * 3 + 2];
  int w = 0;
  while (w < want && nl > 0) {     // k-way merge of the ascending cell lists
    int best = 0;
    for (int l = 1; l < nl; ++l) best = head[l] < head[best] ? l : best;
    const float4 q = sxyz[beg[best]];
    if (pg_hit(ox, oy, oz, q.x, q.y, q.z, r2)) out[w++] = head[best];
    if (++beg[best] == end[best]) {
      --nl;
      beg[best] = beg[nl];
      end[best] = end[nl];
      head[best] = head[nl];
    } else {
      head[best] = __float_as_int(sxyz[beg[best]].w);
    }
  }
}

struct BqLayout {
  PtcCellGridLayout g;
  size_t len, trunc, start, total;
};

BqLayout bq_layout(int64_t n) {
  BqLayout Y;
  PtcArena A;
  const int64_t m = n > 0 ? n : 1;
  Y.g.take_arrays(A, m);
  Y.len = A.take((size_t)m * 4);
  Y.trunc = A.take((size_t)m * 4);
  Y.start = A.take((size_t)m * 8);
  Y.g.take_scratch(A, m, ptc_exclusive_scan_workspace_bytes(m));      // the scan of the lengths runs in it too
  Y.total = A.total;
  return Y;
}

int pg_grid1(int64_t n) { return (int)ptc_cdiv(n > 0 ? n : 1, PG_THREADS); }

// ---------------------------------------------------------------------------------------------------------------------------------
// 2. clustering
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pg_rep(int* __restrict__ parent, int x) {
  int cur = parent[x];
  if (cur != x) {
    int next, prev = x;
    while (cur > (next = parent[cur])) {
      parent[prev] = next;
      prev = cur;
      cur = next;
    }
  }
  return cur;
}

__global__ void pg_cl_init_kernel(int64_t n, int32_t* __restrict__ parent, int32_t* __restrict__ zero4, int64_t n_zero) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) parent[i] = (int32_t)i;
  for (int64_t j = i; j < n_zero; j += (int64_t)gridDim.x * blockDim.x) zero4[j] = 0;
}

// union of every same-label edge of point i; flags bit 0: possibly truncated list, bit 1: no same-label neighbour above i
__global__ void __launch_bounds__(PG_THREADS) pg_hook_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ idx,
                                                             const int32_t* __restrict__ start_len, int64_t n,
                                                             int32_t* __restrict__ parent, int32_t* __restrict__ flags) {
  const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i64 >= n) return;
  const int i = (int)i64;
  const int s = start_len[i64 * 2], len = start_len[i64 * 2 + 1], li = label[i];
  bool low = true;
  for (int e = 0; e < len; ++e) {
    const int j = idx[s + e];
    if (j < 0 || j >= n || j == i || label[j] != li) continue;
    low = low && j < i;
    int a = pg_rep(parent, i), b = pg_rep(parent, j);
    bool again;
    do {
      again = false;
      if (a != b) {
        if (a < b) {
          const int r = atomicCAS(parent + b, b, a);
          if (r != b) { b = r; again = true; }
        } else {
          const int r = atomicCAS(parent + a, a, b);
          if (r != a) { a = r; again = true; }
        }
      }
    } while (again);
  }
  flags[i] = (len >= PG_MAX_NBR ? 1 : 0) | (low ? 2 : 0);
}

__global__ void pg_flatten_kernel(int64_t n, int32_t* __restrict__ parent, const int32_t* __restrict__ flags,
                                  int32_t* __restrict__ compflag, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int x = (int)i;
  while (parent[x] != x) x = parent[x];
  parent[i] = x;
  keys[i] = x;
  if (flags[i] & 1) atomicOr(compflag + x, 1);
}

// component ranges in the member order (sorted by representative, ascending index inside); the list of exact-path components;
// sub[i] = representative (overwritten for the exact components)
__global__ void pg_components_kernel(int64_t n, const int32_t* __restrict__ parent, const int64_t* __restrict__ order,
                                     const int32_t* __restrict__ compflag, int32_t* __restrict__ cstart, int32_t* __restrict__ cend,
                                     int32_t* __restrict__ exlist, int32_t* __restrict__ excount, int32_t* __restrict__ sub) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  sub[p] = parent[p];
  const int r = parent[order[p]];
  if (p == 0 || parent[order[p - 1]] != r) {
    cstart[r] = (int)p;
    if (compflag[r]) exlist[atomicAdd(excount, 1)] = r;
  }
  if (p == n - 1 || parent[order[p + 1]] != r) cend[r] = (int)(p + 1);
}

// the sequential rule of bfs_cluster.cpp:53-100 inside one component per workgroup
__global__ void __launch_bounds__(PG_THREADS) pg_exact_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ idx,
                                                              const int32_t* __restrict__ start_len, int64_t n,
                                                              const int64_t* __restrict__ order, const int32_t* __restrict__ flags,
                                                              const int32_t* __restrict__ cstart, const int32_t* __restrict__ cend,
                                                              const int32_t* __restrict__ exlist, const int32_t* __restrict__ excount,
                                                              int32_t* __restrict__ visited, int32_t* __restrict__ sub,
                                                              int32_t* __restrict__ fa, int32_t* __restrict__ fb) {
  __shared__ int s_first, s_count, s_next;
  const int tid = threadIdx.x;
  const int ncomp = *excount;
  for (int w = blockIdx.x; w < ncomp; w += gridDim.x) {
    const int r = exlist[w];
    const int cs = cstart[r], ce = cend[r];
    int base = cs;
    while (base < ce) {
      if (tid == 0) s_first = 0x7fffffff;
      __syncthreads();
      const int p = base + tid;
      const int m = p < ce ? (int)order[p] : -1;
      const bool unv = m >= 0 && visited[m] == 0;
      if (unv && !(flags[m] & 2)) atomicMin(&s_first, p);
      __syncthreads();
      const int first = s_first;
      if (unv && p < first) {          // singleton seeds: every smaller member is visited, no same-label neighbour above
        visited[m] = 1;
        sub[m] = m;
      }
      if (first == 0x7fffffff) {
        base += blockDim.x;
        __syncthreads();
        continue;
      }
      const int seed = (int)order[first];
      if (tid == 0) {
        visited[seed] = 1;
        sub[seed] = seed;
        fa[cs] = seed;
        s_count = 1;
        s_next = 0;
      }
      __syncthreads();
      int* cur = fa;
      int* nxt = fb;
      while (true) {
        const int cnt = s_count;
        if (cnt == 0) break;
        for (int f = tid; f < cnt; f += blockDim.x) {
          const int u = cur[cs + f];
          const int s = start_len[(int64_t)u * 2], len = start_len[(int64_t)u * 2 + 1], lu = label[u];
          for (int e = 0; e < len; ++e) {
            const int j = idx[s + e];
            if (j < 0 || j >= n || label[j] != lu) continue;
            if (visited[j] == 0 && atomicCAS(visited + j, 0, 1) == 0) {
              sub[j] = seed;
              nxt[cs + atomicAdd(&s_next, 1)] = j;
            }
          }
        }
        __syncthreads();
        if (tid == 0) {
          s_count = s_next;
          s_next = 0;
        }
        __syncthreads();
        int* t = cur;
        cur = nxt;
        nxt = t;
      }
      base = first + 1;
      __syncthreads();
    }
  }
}

__global__ void pg_sizes_kernel(int64_t n, const int32_t* __restrict__ sub, int32_t* __restrict__ size) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(size + sub[i], 1);
}

__global__ void pg_keep_kernel(int64_t n, const int32_t* __restrict__ sub, const int32_t* __restrict__ size, int threshold,
                               const int32_t* __restrict__ label, int skip_negative, int32_t* __restrict__ keep, int32_t* __restrict__ ksize) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool k = sub[i] == (int32_t)i && size[i] >= threshold && !(skip_negative && label[i] < 0);
  keep[i] = k ? 1 : 0;
  ksize[i] = k ? size[i] : 0;
}

__global__ void pg_cluster_keys_kernel(int64_t n, const int32_t* __restrict__ sub, const int32_t* __restrict__ keep,
                                       const int64_t* __restrict__ cid, const int32_t* __restrict__ ksize,
                                       const int64_t* __restrict__ koff, int64_t* __restrict__ keys, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = sub[i];
  keys[i] = keep[s] ? cid[s] : n;
  if (i == n - 1) {
    counts[0] = (int32_t)(cid[i] + keep[i]);
    counts[1] = (int32_t)(koff[i] + ksize[i]);
  }
}

__global__ void pg_cluster_fill_kernel(int64_t n, const int64_t* __restrict__ order, const int64_t* __restrict__ keys,
                                       const int32_t* __restrict__ keep, const int64_t* __restrict__ cid,
                                       const int64_t* __restrict__ koff, int64_t n_cluster, int64_t n_sum,
                                       int32_t* __restrict__ cidx, int32_t* __restrict__ coff) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  if (p < n_sum) {
    const int64_t i = order[p];
    cidx[p * 2] = (int32_t)keys[i];
    cidx[p * 2 + 1] = (int32_t)i;
  }
  if (keep[p]) {
    const int64_t c = cid[p];
    if (c < n_cluster) coff[c] = (int32_t)koff[p];
  }
  if (p == 0) coff[n_cluster] = (int32_t)n_sum;
}

struct ClLayout {
  size_t parent, flags, compflag, visited, size, excount, sub, keep, ksize, cstart, cend, exlist, fa, fb, cid, koff, keys, order,
      scratch, total;
};

ClLayout cl_layout(int64_t n) {
  ClLayout Y;
  PtcArena A;
  const int64_t m = n > 0 ? n : 1;
  Y.parent = A.take((size_t)m * 4);
  Y.flags = A.take((size_t)m * 16 + 4);      // flags .. excount are one piece, zeroed by the init kernel
  Y.compflag = Y.flags + (size_t)m * 4;
  Y.visited = Y.compflag + (size_t)m * 4;
  Y.size = Y.visited + (size_t)m * 4;
  Y.excount = Y.size + (size_t)m * 4;
  Y.sub = A.take((size_t)m * 4);
  Y.keep = A.take((size_t)m * 4);
  Y.ksize = A.take((size_t)m * 4);
  Y.cstart = A.take((size_t)m * 4);
  Y.cend = A.take((size_t)m * 4);
  Y.exlist = A.take((size_t)m * 4);
  Y.fa = A.take((size_t)m * 4);
  Y.fb = A.take((size_t)m * 4);
  Y.cid = A.take((size_t)m * 8);
  Y.koff = A.take((size_t)m * 8);
  Y.keys = A.take((size_t)m * 8);
  Y.order = A.take((size_t)m * 8);
  size_t s1 = ptc_sort_keys_workspace_bytes(m, 1), s2 = ptc_exclusive_scan_workspace_bytes(m);
  Y.scratch = A.take(s1 > s2 ? s1 : s2);
  Y.total = A.total;
  return Y;
}

int pg_bits(int64_t v) {
  int b = 1;
  while (b < 62 && (int64_t(1) << b) <= v) ++b;
  return b;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3. proposal scores and masks
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(PG_THREADS) pg_scores_kernel(const T* __restrict__ logits, int c, const int32_t* __restrict__ label,
                                                               const int32_t* __restrict__ cidx, const int32_t* __restrict__ coff,
                                                               const int64_t* __restrict__ point_map, int32_t* __restrict__ count,
                                                               int32_t* __restrict__ cls, float* __restrict__ score) {
  __shared__ float red[PG_THREADS];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int beg = coff[k], end = coff[k + 1];
  const int seed = cidx[(int64_t)beg * 2 + 1];
  const int cl = label[seed];
  float acc = 0.f;
  for (int m = beg + tid; m < end; m += PG_THREADS) {
    const int pt = cidx[(int64_t)m * 2 + 1];
    const int64_t row = point_map ? point_map[pt] : (int64_t)pt;
    const T* lr = logits + row * c;
    float mx = -__builtin_inff();
    for (int j = 0; j < c; ++j) mx = fmaxf(mx, ptc_to_float(lr[j]));
    float sum = 0.f;
    for (int j = 0; j < c; ++j) sum += expf(ptc_to_float(lr[j]) - mx);
    acc += expf(ptc_to_float(lr[cl]) - mx) / sum;
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = PG_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    count[k] = end - beg;
    cls[k] = cl;
    score[k] = red[0] / (float)(end - beg);
  }
}

// out[row[k], point_map[member]] = 1 for every member of a cluster k with row[k] >= 0 (out zeroed by the caller)
__global__ void pg_masks_kernel(const int32_t* __restrict__ cidx, int64_t n_sum, const int64_t* __restrict__ row,
                                const int64_t* __restrict__ point_map, int64_t n_points, int32_t* __restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_sum) return;
  const int64_t r = row[cidx[m * 2]];
  if (r < 0) return;
  const int pt = cidx[m * 2 + 1];
  const int64_t col = point_map ? point_map[pt] : (int64_t)pt;
  out[r * n_points + col] = 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 4. bias losses
// ---------------------------------------------------------------------------------------------------------------------------------
#define PG_LOSS_BLOCKS 1024
#define PG_EPS 1e-8f

template <typename T>
__device__ __forceinline__ void pg_bias_row(const T* __restrict__ bp, const float* __restrict__ coord, const float* __restrict__ cen,
                                            int64_t i, float (&p)[3], float (&g)[3]) {
  for (int a = 0; a < 3; ++a) {
    p[a] = ptc_to_float(bp[i * 3 + a]);
    g[a] = cen[i * 3 + a] - coord[i * 3 + a];
  }
}

__device__ __forceinline__ float pg_norm3(const float (&v)[3]) { return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

template <typename T>
__global__ void __launch_bounds__(PG_THREADS) pg_bias_fwd_kernel(const T* __restrict__ bp, const float* __restrict__ coord,
                                                                 const float* __restrict__ cen, const int64_t* __restrict__ inst,
                                                                 int64_t n, int64_t ignore, float* __restrict__ part,
                                                                 int32_t* __restrict__ pcount) {
  __shared__ float s_l1[PG_THREADS], s_cos[PG_THREADS];
  __shared__ int s_m[PG_THREADS];
  const int tid = threadIdx.x;
  float l1 = 0.f, cs = 0.f;
  int cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * PG_THREADS + tid; i < n; i += (int64_t)gridDim.x * PG_THREADS) {
    if (inst[i] == ignore) continue;
    float p[3], g[3];
    pg_bias_row(bp, coord, cen, i, p, g);
    l1 += fabsf(p[0] - g[0]) + fabsf(p[1] - g[1]) + fabsf(p[2] - g[2]);
    const float dp = pg_norm3(p) + PG_EPS, dg = pg_norm3(g) + PG_EPS;
    cs += -((p[0] / dp) * (g[0] / dg) + (p[1] / dp) * (g[1] / dg) + (p[2] / dp) * (g[2] / dg));
    ++cnt;
  }
  s_l1[tid] = l1;
  s_cos[tid] = cs;
  s_m[tid] = cnt;
  __syncthreads();
  for (int s = PG_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      s_l1[tid] += s_l1[tid + s];
      s_cos[tid] += s_cos[tid + s];
      s_m[tid] += s_m[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[blockIdx.x * 2] = s_l1[0];
    part[blockIdx.x * 2 + 1] = s_cos[0];
    pcount[blockIdx.x] = s_m[0];
  }
}

// out = (l1, cos, sum(mask)); one workgroup, fixed order over the per-block partials
__global__ void __launch_bounds__(PG_THREADS) pg_bias_final_kernel(const float* __restrict__ part, const int32_t* __restrict__ pcount,
                                                                   int nb, float* __restrict__ out) {
  __shared__ float s_l1[PG_THREADS], s_cos[PG_THREADS];
  __shared__ long long s_m[PG_THREADS];
  const int tid = threadIdx.x;
  float l1 = 0.f, cs = 0.f;
  long long m = 0;
  for (int b = tid; b < nb; b += PG_THREADS) {
    l1 += part[b * 2];
    cs += part[b * 2 + 1];
    m += pcount[b];
  }
  s_l1[tid] = l1;
  s_cos[tid] = cs;
  s_m[tid] = m;
  __syncthreads();
  for (int s = PG_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      s_l1[tid] += s_l1[tid + s];
      s_cos[tid] += s_cos[tid + s];
      s_m[tid] += s_m[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float msum = (float)s_m[0];
    out[0] = s_l1[0] / (msum + PG_EPS);
    out[1] = s_cos[0] / (msum + PG_EPS);
    out[2] = msum;
  }
}

template <typename T>
__global__ void pg_bias_bwd_kernel(const T* __restrict__ bp, const float* __restrict__ coord, const float* __restrict__ cen,
                                   const int64_t* __restrict__ inst, int64_t n, int64_t ignore, const float* __restrict__ dout,
                                   const float* __restrict__ fwd, T* __restrict__ dbp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float d[3] = {0.f, 0.f, 0.f};
  if (inst[i] != ignore) {
    const float w = 1.f / (fwd[2] + PG_EPS);
    const float wl1 = dout[0] * w, wcos = dout[1] * w;
    float p[3], g[3];
    pg_bias_row(bp, coord, cen, i, p, g);
    const float s = pg_norm3(p), dp = s + PG_EPS, dg = pg_norm3(g) + PG_EPS;
    float gn[3], pg = 0.f;
    for (int a = 0; a < 3; ++a) {
      gn[a] = g[a] / dg;
      pg += p[a] * gn[a];
    }
    const float c2 = s > 0.f ? pg / (dp * dp) / s : 0.f;   // torch's norm backward is 0 at a zero row
    for (int a = 0; a < 3; ++a) {
      const float df = p[a] - g[a];
      const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
      d[a] = wl1 * sg - wcos * (gn[a] / dp - c2 * p[a]);
    }
  }
  for (int a = 0; a < 3; ++a) dbp[i * 3 + a] = ptc_from_float<T>(d[a]);
}

}  // namespace

// =================================================================================================================================
extern "C" size_t ptc_pg_ball_query_workspace_bytes(int64_t n) { return bq_layout(n).total; }

extern "C" int ptc_pg_ball_query_count(const float* xyz, const int32_t* batch_idxs, int64_t n, int n_batch, float radius,
                                       int32_t* start_len, int64_t* total, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && n < (1ll << 31), PTC_EINVAL, "ptc_pg_ball_query_count: n=%lld", (long long)n);
  PTC_REQUIRE(n_batch >= 0 && n_batch < 32768, PTC_EUNSUPPORTED, "ptc_pg_ball_query_count: %d batch segments (at most 32767)", n_batch);
  PTC_REQUIRE(total && workspace && (n == 0 || (xyz && batch_idxs && start_len)), PTC_EINVAL, "ptc_pg_ball_query_count: null buffer");
  const BqLayout Y = bq_layout(n);
  PTC_REQUIRE(workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_pg_ball_query_count: workspace %zu < %zu", workspace_bytes, Y.total);
  hipStream_t s = (hipStream_t)stream;
  PTC_HIP(hipMemsetAsync(total, 0, 16, s));
  if (n == 0) return PTC_OK;
  char* ws = (char*)workspace;
  const float rabs = fabsf(radius);
  if (!(rabs > 0.f)) {                  // radius 0 / NaN: d2 < r2 never holds
    PTC_HIP(hipMemsetAsync(start_len, 0, (size_t)n * 8, s));
    return PTC_OK;
  }
  PtcCellGrid* grid = (PtcCellGrid*)(ws + Y.g.grid);
  int rc = ptc_cell_grid_params(xyz, n, (double)rabs, (uint32_t*)(ws + Y.g.mm), grid, stream);
  if (rc != PTC_OK) return rc;
  const int g1 = pg_grid1(n);
  int64_t* keys = (int64_t*)(ws + Y.g.keys);
  int64_t* skeys = (int64_t*)(ws + Y.g.skeys);
  float4* sxyz = (float4*)(ws + Y.g.sxyz);
  int32_t* len = (int32_t*)(ws + Y.len);
  int32_t* trunc = (int32_t*)(ws + Y.trunc);
  int64_t* start = (int64_t*)(ws + Y.start);
  hipLaunchKernelGGL(pg_keys_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, xyz, batch_idxs, n, n_batch, (const PtcCellGrid*)grid, keys);
  PTC_CHECK_LAUNCH("pg_keys_kernel");
  rc = ptc_cell_grid_sort(xyz, keys, n, 63, (int64_t*)(ws + Y.g.order), skeys, sxyz, ws + Y.g.scratch, Y.g.scratch_bytes, stream);
  if (rc != PTC_OK) return rc;
  const float r2 = radius * radius;
  hipLaunchKernelGGL(pg_count_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, xyz, (const int64_t*)keys, (const int64_t*)skeys,
                     (const float4*)sxyz, n, r2, len, trunc);
  PTC_CHECK_LAUNCH("pg_count_kernel");
  rc = ptc_exclusive_scan_i32(len, n, start, ws + Y.g.scratch, ptc_exclusive_scan_workspace_bytes(n), stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(pg_start_len_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, (const int32_t*)len, (const int32_t*)trunc,
                     (const int64_t*)start, n, start_len, total);
  PTC_CHECK_LAUNCH("pg_start_len_kernel");
  return PTC_OK;
}

extern "C" int ptc_pg_ball_query_fill(const float* xyz, int64_t n, float radius, const int32_t* start_len, int32_t* idx,
                                      void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && n < (1ll << 31), PTC_EINVAL, "ptc_pg_ball_query_fill: n=%lld", (long long)n);
  const BqLayout Y = bq_layout(n);
  PTC_REQUIRE(workspace && workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_pg_ball_query_fill: workspace %zu < %zu", workspace_bytes, Y.total);
  if (n == 0 || !(fabsf(radius) > 0.f)) return PTC_OK;
  PTC_REQUIRE(xyz && start_len && idx, PTC_EINVAL, "ptc_pg_ball_query_fill: null buffer");
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(pg_fill_kernel, dim3((unsigned)pg_grid1(n)), dim3(PG_THREADS), 0, (hipStream_t)stream, xyz,
                     (const int64_t*)(ws + Y.g.keys), (const int64_t*)(ws + Y.g.skeys), (const float4*)(ws + Y.g.sxyz), n, radius * radius,
                     start_len, idx);
  PTC_CHECK_LAUNCH("pg_fill_kernel");
  return PTC_OK;
}

extern "C" size_t ptc_pg_cluster_workspace_bytes(int64_t n) { return cl_layout(n).total; }

extern "C" int ptc_pg_cluster_count(const int32_t* label, const int32_t* idx, const int32_t* start_len, int64_t n, int threshold,
                                    int skip_negative, int32_t* counts, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && n < (1ll << 31), PTC_EINVAL, "ptc_pg_cluster_count: n=%lld", (long long)n);
  PTC_REQUIRE(counts && workspace && (n == 0 || (label && start_len)), PTC_EINVAL, "ptc_pg_cluster_count: null buffer");
  const ClLayout Y = cl_layout(n);
  PTC_REQUIRE(workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_pg_cluster_count: workspace %zu < %zu", workspace_bytes, Y.total);
  hipStream_t s = (hipStream_t)stream;
  PTC_HIP(hipMemsetAsync(counts, 0, 8, s));
  if (n == 0) return PTC_OK;
  char* ws = (char*)workspace;
  int32_t* parent = (int32_t*)(ws + Y.parent);
  int32_t* flags = (int32_t*)(ws + Y.flags);
  int32_t* compflag = (int32_t*)(ws + Y.compflag);
  int32_t* visited = (int32_t*)(ws + Y.visited);
  int32_t* size = (int32_t*)(ws + Y.size);
  int32_t* excount = (int32_t*)(ws + Y.excount);
  int32_t* sub = (int32_t*)(ws + Y.sub);
  int32_t* keep = (int32_t*)(ws + Y.keep);
  int32_t* ksize = (int32_t*)(ws + Y.ksize);
  int32_t* cstart = (int32_t*)(ws + Y.cstart);
  int32_t* cend = (int32_t*)(ws + Y.cend);
  int32_t* exlist = (int32_t*)(ws + Y.exlist);
  int64_t* cid = (int64_t*)(ws + Y.cid);
  int64_t* koff = (int64_t*)(ws + Y.koff);
  int64_t* keys = (int64_t*)(ws + Y.keys);
  int64_t* order = (int64_t*)(ws + Y.order);
  const int g1 = pg_grid1(n);
  hipLaunchKernelGGL(pg_cl_init_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, n, parent, flags, 4 * n + 1);
  PTC_CHECK_LAUNCH("pg_cl_init_kernel");
  hipLaunchKernelGGL(pg_hook_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, label, idx, start_len, n, parent, flags);
  PTC_CHECK_LAUNCH("pg_hook_kernel");
  hipLaunchKernelGGL(pg_flatten_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, n, parent, (const int32_t*)flags, compflag, keys);
  PTC_CHECK_LAUNCH("pg_flatten_kernel");
  const int bits = pg_bits(n);
  int rc = ptc_sort_keys(keys, n, 1, 0, bits, order, nullptr, ws + Y.scratch, ptc_sort_keys_workspace_bytes(n, 1), stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(pg_components_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, n, (const int32_t*)parent, (const int64_t*)order,
                     (const int32_t*)compflag, cstart, cend, exlist, excount, sub);
  PTC_CHECK_LAUNCH("pg_components_kernel");
  const int gx = g1 < 1024 ? g1 : 1024;
  hipLaunchKernelGGL(pg_exact_kernel, dim3((unsigned)gx), dim3(PG_THREADS), 0, s, label, idx, start_len, n, (const int64_t*)order,
                     (const int32_t*)flags, (const int32_t*)cstart, (const int32_t*)cend, (const int32_t*)exlist, (const int32_t*)excount,
                     visited, sub, (int32_t*)(ws + Y.fa), (int32_t*)(ws + Y.fb));
  PTC_CHECK_LAUNCH("pg_exact_kernel");
  hipLaunchKernelGGL(pg_sizes_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, n, (const int32_t*)sub, size);
  PTC_CHECK_LAUNCH("pg_sizes_kernel");
  hipLaunchKernelGGL(pg_keep_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, n, (const int32_t*)sub, (const int32_t*)size, threshold,
                     label, skip_negative, keep, ksize);
  PTC_CHECK_LAUNCH("pg_keep_kernel");
  const size_t scw = ptc_exclusive_scan_workspace_bytes(n);
  rc = ptc_exclusive_scan_i32(keep, n, cid, ws + Y.scratch, scw, stream);
  if (rc != PTC_OK) return rc;
  rc = ptc_exclusive_scan_i32(ksize, n, koff, ws + Y.scratch, scw, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(pg_cluster_keys_kernel, dim3((unsigned)g1), dim3(PG_THREADS), 0, s, n, (const int32_t*)sub, (const int32_t*)keep,
                     (const int64_t*)cid, (const int32_t*)ksize, (const int64_t*)koff, keys, counts);
  PTC_CHECK_LAUNCH("pg_cluster_keys_kernel");
  return ptc_sort_keys(keys, n, 1, 0, pg_bits(n), order, nullptr, ws + Y.scratch, ptc_sort_keys_workspace_bytes(n, 1), stream);
}

extern "C" int ptc_pg_cluster_fill(int64_t n, int64_t n_cluster, int64_t n_sum, int32_t* cluster_idxs, int32_t* cluster_offsets,
                                   void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && n < (1ll << 31) && n_cluster >= 0 && n_cluster <= n && n_sum >= 0 && n_sum <= n, PTC_EINVAL,
              "ptc_pg_cluster_fill: n=%lld n_cluster=%lld n_sum=%lld", (long long)n, (long long)n_cluster, (long long)n_sum);
  const ClLayout Y = cl_layout(n);
  PTC_REQUIRE(workspace && workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_pg_cluster_fill: workspace %zu < %zu", workspace_bytes, Y.total);
  PTC_REQUIRE(cluster_offsets && (n_sum == 0 || cluster_idxs), PTC_EINVAL, "ptc_pg_cluster_fill: null buffer");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    PTC_HIP(hipMemsetAsync(cluster_offsets, 0, 4, s));
    return PTC_OK;
  }
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(pg_cluster_fill_kernel, dim3((unsigned)pg_grid1(n)), dim3(PG_THREADS), 0, s, n, (const int64_t*)(ws + Y.order),
                     (const int64_t*)(ws + Y.keys), (const int32_t*)(ws + Y.keep), (const int64_t*)(ws + Y.cid),
                     (const int64_t*)(ws + Y.koff), n_cluster, n_sum, cluster_idxs, cluster_offsets);
  PTC_CHECK_LAUNCH("pg_cluster_fill_kernel");
  return PTC_OK;
}

extern "C" int ptc_pg_proposal_scores(const void* logits, int dtype, int64_t n_rows, int c, const int32_t* label,
                                      const int32_t* cluster_idxs, const int32_t* cluster_offsets, int64_t n_cluster,
                                      const int64_t* point_map, int32_t* count, int32_t* cls, float* score, ptc_stream_t stream) {
  PTC_REQUIRE(n_cluster >= 0 && n_cluster < (1ll << 31) && c >= 1 && n_rows >= 0, PTC_EINVAL, "ptc_pg_proposal_scores: n_cluster=%lld c=%d",
              (long long)n_cluster, c);
  if (n_cluster == 0) return PTC_OK;
  PTC_REQUIRE(logits && label && cluster_idxs && cluster_offsets && count && cls && score, PTC_EINVAL, "ptc_pg_proposal_scores: null buffer");
  PTC_DISPATCH_DTYPE(dtype, T, {
    hipLaunchKernelGGL(pg_scores_kernel<T>, dim3((unsigned)n_cluster), dim3(PG_THREADS), 0, (hipStream_t)stream, (const T*)logits, c, label,
                       cluster_idxs, cluster_offsets, point_map, count, cls, score);
    PTC_CHECK_LAUNCH("pg_scores_kernel");
  });
  return PTC_OK;
}

extern "C" int ptc_pg_proposal_masks(const int32_t* cluster_idxs, int64_t n_sum, const int64_t* row, const int64_t* point_map,
                                     int64_t n_points, int64_t n_rows_out, int32_t* out, ptc_stream_t stream) {
  PTC_REQUIRE(n_sum >= 0 && n_points >= 0 && n_rows_out >= 0, PTC_EINVAL, "ptc_pg_proposal_masks: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows_out * n_points == 0) return PTC_OK;
  PTC_REQUIRE(out && (n_sum == 0 || (cluster_idxs && row)), PTC_EINVAL, "ptc_pg_proposal_masks: null buffer");
  PTC_HIP(hipMemsetAsync(out, 0, (size_t)n_rows_out * n_points * 4, s));
  if (n_sum == 0) return PTC_OK;
  hipLaunchKernelGGL(pg_masks_kernel, dim3((unsigned)pg_grid1(n_sum)), dim3(PG_THREADS), 0, s, cluster_idxs, n_sum, row, point_map,
                     n_points, out);
  PTC_CHECK_LAUNCH("pg_masks_kernel");
  return PTC_OK;
}

extern "C" size_t ptc_pg_bias_loss_workspace_bytes(int64_t n) {
  (void)n;
  return (size_t)PG_LOSS_BLOCKS * 12;
}

extern "C" int ptc_pg_bias_loss_fwd(const void* bias_pred, int dtype, const float* coord, const float* centroid, const int64_t* instance,
                                    int64_t n, int64_t ignore_index, float* out, void* workspace, size_t workspace_bytes,
                                    ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0, PTC_EINVAL, "ptc_pg_bias_loss_fwd: n=%lld", (long long)n);
  PTC_REQUIRE(out && workspace && (n == 0 || (bias_pred && coord && centroid && instance)), PTC_EINVAL, "ptc_pg_bias_loss_fwd: null buffer");
  PTC_REQUIRE(workspace_bytes >= ptc_pg_bias_loss_workspace_bytes(n), PTC_EWORKSPACE, "ptc_pg_bias_loss_fwd: workspace %zu", workspace_bytes);
  hipStream_t s = (hipStream_t)stream;
  int64_t nb64 = ptc_cdiv(n > 0 ? n : 1, PG_THREADS);
  const int nb = (int)(nb64 > PG_LOSS_BLOCKS ? PG_LOSS_BLOCKS : nb64);
  float* part = (float*)workspace;
  int32_t* pcount = (int32_t*)((char*)workspace + (size_t)PG_LOSS_BLOCKS * 8);
  PTC_DISPATCH_DTYPE(dtype, T, {
    hipLaunchKernelGGL(pg_bias_fwd_kernel<T>, dim3((unsigned)nb), dim3(PG_THREADS), 0, s, (const T*)bias_pred, coord, centroid, instance, n,
                       ignore_index, part, pcount);
    PTC_CHECK_LAUNCH("pg_bias_fwd_kernel");
  });
  hipLaunchKernelGGL(pg_bias_final_kernel, dim3(1), dim3(PG_THREADS), 0, s, (const float*)part, (const int32_t*)pcount, nb, out);
  PTC_CHECK_LAUNCH("pg_bias_final_kernel");
  return PTC_OK;
}

extern "C" int ptc_pg_bias_loss_bwd(const void* bias_pred, int dtype, const float* coord, const float* centroid, const int64_t* instance,
                                    int64_t n, int64_t ignore_index, const float* dout, const float* fwd_out, void* dbias_pred,
                                    ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0, PTC_EINVAL, "ptc_pg_bias_loss_bwd: n=%lld", (long long)n);
  if (n == 0) return PTC_OK;
  PTC_REQUIRE(bias_pred && coord && centroid && instance && dout && fwd_out && dbias_pred, PTC_EINVAL, "ptc_pg_bias_loss_bwd: null buffer");
  PTC_DISPATCH_DTYPE(dtype, T, {
    hipLaunchKernelGGL(pg_bias_bwd_kernel<T>, dim3((unsigned)pg_grid1(n)), dim3(PG_THREADS), 0, (hipStream_t)stream, (const T*)bias_pred,
                       coord, centroid, instance, n, ignore_index, dout, fwd_out, (T*)dbias_pred);
    PTC_CHECK_LAUNCH("pg_bias_bwd_kernel");
  });
  return PTC_OK;
}
