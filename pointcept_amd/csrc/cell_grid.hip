// cell_grid.hip -- the kernels and host steps of cell_grid.h that are the same for every caller.
#include "cell_grid.h"

#define CG_THREADS 256

namespace {

// componentwise min / max of the finite rows (order-preserving integer codes, integer atomics); hi == 0: no finite row seen
__global__ void cg_bounds_kernel(const float* __restrict__ xyz, int64_t n, uint32_t* __restrict__ mm) {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
    if (!ptc_finite3(x, y, z)) continue;
    const uint32_t e[3] = {ptc_float_enc(x), ptc_float_enc(y), ptc_float_enc(z)};
    for (int a = 0; a < 3; ++a) {
      lo[a] = e[a] < lo[a] ? e[a] : lo[a];
      hi[a] = e[a] > hi[a] ? e[a] : hi[a];
    }
  }
  for (int a = 0; a < 3; ++a) {
    if (hi[a] == 0u) continue;        // this thread saw no finite point
    atomicMin(mm + a, lo[a]);
    atomicMax(mm + 3 + a, hi[a]);
  }
}

__global__ void cg_params_kernel(const uint32_t* __restrict__ mm, double radius, PtcCellGrid* __restrict__ g) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double ext = 0.0;
  const bool any = mm[3] != 0u;
  for (int a = 0; a < 3; ++a) {
    const double lo = any ? (double)ptc_float_dec(mm[a]) : 0.0, hi = any ? (double)ptc_float_dec(mm[3 + a]) : 0.0;
    g->mn[a] = lo;
    ext = hi - lo > ext ? hi - lo : ext;
  }
  double edge = radius * PTC_EDGE_MARGIN;
  if (ext / edge > PTC_EXTENT_CELLS) edge = ext / PTC_EXTENT_CELLS;
  g->edge = edge;
}

// sxyz[p] = (xyz[order[p]], bits of order[p])
__global__ void cg_sorted_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ order, int64_t n, float4* __restrict__ sxyz) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t k = order[p];
  sxyz[p] = make_float4(xyz[k * 3], xyz[k * 3 + 1], xyz[k * 3 + 2], __int_as_float((int)k));
}

int cg_grid1(int64_t n) { return (int)ptc_cdiv(n > 0 ? n : 1, CG_THREADS); }

}  // namespace

int ptc_cell_grid_params(const float* xyz, int64_t n, double radius, uint32_t* mm, PtcCellGrid* grid, ptc_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  PTC_HIP(hipMemsetAsync(mm, 0xff, 12, s));
  PTC_HIP(hipMemsetAsync(mm + 3, 0, 12, s));
  const int g1 = cg_grid1(n);
  hipLaunchKernelGGL(cg_bounds_kernel, dim3((unsigned)(g1 > 1024 ? 1024 : g1)), dim3(CG_THREADS), 0, s, xyz, n, mm);
  PTC_CHECK_LAUNCH("cg_bounds_kernel");
  hipLaunchKernelGGL(cg_params_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)mm, radius, grid);
  PTC_CHECK_LAUNCH("cg_params_kernel");
  return PTC_OK;
}

int ptc_cell_grid_sort(const float* xyz, const int64_t* keys, int64_t n, int end_bit, int64_t* order, int64_t* sorted_keys, float4* sxyz,
                       void* scratch, size_t scratch_bytes, ptc_stream_t stream) {
  const int rc = ptc_sort_keys_ex(keys, n, 1, 0, end_bit, order, nullptr, sorted_keys, scratch, scratch_bytes, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(cg_sorted_kernel, dim3((unsigned)cg_grid1(n)), dim3(CG_THREADS), 0, (hipStream_t)stream, xyz, (const int64_t*)order, n,
                     sxyz);
  PTC_CHECK_LAUNCH("cg_sorted_kernel");
  return PTC_OK;
}
