// cell_grid.h -- the uniform cell grid behind the radius queries (pg_cluster.hip's ball query, msc.hip's view matching).
//
// A point cloud is sorted into cells of edge >= radius * (1 + 1e-4), grown when the extent would overflow the 16-bit cell fields of the
// packed key (scene << 48 | cz << 32 | cy << 16 | cx); a query then visits the 27 cells around its own as up to 9 runs of the sorted keys
// (x contiguous).  The sort is stable, so the points of a cell are ascending by index.  Host side (cell_grid.hip, declared in
// ptc_common.h): ptc_cell_grid_params -> the caller's own keys kernel (scene and sentinel are the caller's, cell and key packing are
// ptc_cell / ptc_cell_key) -> ptc_cell_grid_sort.
#pragma once
#include "ptc_common.h"

#define PTC_CELL_MAX 65533           // cell fields hold 0..65535; neighbours reach -1..65534
#define PTC_EXTENT_CELLS 60000.0
#define PTC_EDGE_MARGIN 1.0001       // cell edge >= radius * (1 + 1e-4): the fp32 rounding of d2 and of the root never reaches past one cell

struct PtcCellGrid {                 // written by ptc_cell_grid_params
  double mn[3];
  double edge;
};

__device__ __forceinline__ bool ptc_finite3(float x, float y, float z) {
  return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

__device__ __forceinline__ int ptc_cell(float v, double mn, double edge) {
  double c = floor(((double)v - mn) / edge);
  c = c < 0.0 ? 0.0 : (c > (double)PTC_CELL_MAX ? (double)PTC_CELL_MAX : c);
  return (int)c;
}

__device__ __forceinline__ int64_t ptc_cell_key(int b, int cx, int cy, int cz) {
  return ((int64_t)b << 48) | ((int64_t)cz << 32) | ((int64_t)cy << 16) | (int64_t)cx;
}

__device__ __forceinline__ int64_t ptc_lower_bound(const int64_t* __restrict__ a, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// f(lo, hi, cy', cz') for each of the up to 9 x-runs of the 27 cells around (cx, cy, cz) of scene b: sorted positions [lo, hi) hold the
// cells max(cx - 1, 0) .. cx + 1 of row (cy', cz'); dz outer, dy inner
template <typename F>
__device__ __forceinline__ void ptc_cell_runs(const int64_t* __restrict__ skeys, int64_t n, int b, int cx, int cy, int cz, F&& f) {
  for (int dz = -1; dz <= 1; ++dz) {
    if (cz + dz < 0) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      if (cy + dy < 0) continue;
      const int x0 = cx > 0 ? cx - 1 : 0;
      const int64_t lo = ptc_lower_bound(skeys, 0, n, ptc_cell_key(b, x0, cy + dy, cz + dz));
      const int64_t hi = ptc_lower_bound(skeys, lo, n, ptc_cell_key(b, cx + 2, cy + dy, cz + dz));
      f(lo, hi, cy + dy, cz + dz);
    }
  }
}

// the grid's part of a workspace: the arrays first, the sort scratch (at least `min_scratch` bytes) wherever the caller's own arrays end
struct PtcCellGridLayout {
  size_t mm, grid, keys, order, skeys, sxyz, scratch, scratch_bytes;
  void take_arrays(PtcArena& A, int64_t m) {
    mm = A.take(6 * 4);
    grid = A.take(sizeof(PtcCellGrid));
    keys = A.take((size_t)m * 8);
    order = A.take((size_t)m * 8);
    skeys = A.take((size_t)m * 8);
    sxyz = A.take((size_t)m * 16);
  }
  void take_scratch(PtcArena& A, int64_t m, size_t min_scratch = 0) {
    const size_t s = ptc_sort_keys_workspace_bytes(m, 1);
    scratch = A.take(s > min_scratch ? s : min_scratch);
    scratch_bytes = A.total - scratch;
  }
};
