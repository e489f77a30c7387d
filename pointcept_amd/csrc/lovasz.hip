// lovasz.hip -- Lovasz-Softmax loss (multiclass, classes = "present", whole batch) forward + gradient.
//
// Replaces LovaszLoss(mode="multiclass", ignore_index) of pointcept/models/losses/lovasz.py:118-146 (_lovasz_softmax_flat),
// :22-33 (_lovasz_grad), :149-166 (_flatten_probas) as configured at configs/scannet/semseg-pt-v3m1-0-base.py:49-52 and
// called from pointcept/models/default.py:78-84.  The reference loops over the classes present in the labels and, for
// each, runs softmax column -> |fg - p| -> torch.sort(descending) -> cumsum -> Jaccard differences -> dot: 20 sorts
// of N floats plus ~12 elementwise launches per class.  Here the whole loss is six launches around ONE segmented
// radix sort of the [C, N] error matrix (the row-batched sort of scan_sort.hip that also orders the serialization
// curves):
//   1. lovasz_keys      : per point softmax in fp32 straight from the (strided, 16-bit) head output; key[c][i] =
//                         (0x3f800000 - bits(|fg - p_c|)) << 1 | fg: errors lie in [0, 1], so the 30-bit integer ascends as the
//                         error descends.  Ignored points get error 0 (they sort to the tail and multiply their
//                         Jaccard step by 0).  Class populations are counted with integer atomics (exact, order free).
//   2. ptc_sort_keys_ex : C rows of N keys, bits [1, 31): 4 passes; the foreground flag in bit 0 is a payload the sort carries along,
//                         and the sorted key words come back with the order (round 5: the first form gathered target[order[t]] for the
//                         flag and keys[order[t]] for the error -- two random 8-byte gathers per slot, 143 + 452 us at 819200 x 20,
//                         1.8 GB of sector traffic in lovasz_step for 0.5 GB of operands, profiles/r04_zy_step_traffic.txt).
//   3. lovasz_fg        : foreground flag of every sorted slot (bit 0 of its key); ptc_exclusive_scan_i32 over the flat [C*N] flags.
//   4. lovasz_step      : Jaccard step of slot i, computed EXACTLY from the integer counts instead of as the difference
//                         of two nearly equal quotients (lovasz.py:31-32): with I = fg still to come, U = union so far,
//                         step = 1/U for a foreground slot and I/(U (U-1)) for a background slot.  Accumulates
//                         error * step per workgroup (fixed order, no float atomics) and writes the gradient w.r.t.
//                         the probability back to the point: g[c][src] = -+ step / n_present.
//   5. lovasz_finish    : sums the partials in a fixed order -> loss.
//   6. lovasz_dlogits   : softmax backward per point, dz = p * (g - <g, p>), 0 for ignored points.
// All of it is HBM-bound streaming work (~190 B per (point, class) slot); bit-reproducible.
#include "ptc_common.h"
#include "voxel_keys.h"
#include "loss_rows.h"

#define LV_THREADS 256
#define LV_MAX_C PTC_LOVASZ_DENSE_MAX_C
#define LV_ONE 0x3f800000u
#define LV_STEP_BLOCKS 4096

// key word of one (class, point) slot: bits [1, 31) ascend as the error descends, bit 0 = the slot is foreground (its point carries this
// class) -- below the sorted bit range, carried along by the sort
__device__ __forceinline__ int64_t lv_key(float e, bool fg) { return (int64_t)(((uint64_t)(LV_ONE - __float_as_uint(e)) << 1) | (fg ? 1u : 0u)); }
__device__ __forceinline__ float lv_key_error(int64_t key) { return __uint_as_float(LV_ONE - (uint32_t)((uint64_t)key >> 1)); }

template <typename T>
__global__ void __launch_bounds__(LV_THREADS)
lovasz_keys_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target, int64_t n, int c,
                   int64_t ignore_index, int64_t* __restrict__ keys, int32_t* __restrict__ class_count) {
  __shared__ int32_t cnt[LV_MAX_C];
  if (threadIdx.x < LV_MAX_C) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (i < n) {
    const T* row = logits + i * row_stride;
    const int64_t t = target[i];
    const bool valid = t != ignore_index && t >= 0 && t < c;
    float m = -INFINITY;
    for (int j = 0; j < c; ++j) m = fmaxf(m, ptc_to_float(row[j]));
    float ssum = 0.f;
    for (int j = 0; j < c; ++j) ssum += __expf(ptc_to_float(row[j]) - m);
    const float inv = 1.f / ssum;
    for (int j = 0; j < c; ++j) {
      const float p = __expf(ptc_to_float(row[j]) - m) * inv;
      float e = valid ? (j == t ? 1.f - p : p) : 0.f;
      e = fminf(fmaxf(e, 0.f), 1.f);
      keys[(int64_t)j * n + i] = lv_key(e, valid && j == t);
    }
    if (valid) atomicAdd(&cnt[(int)t], 1);
  }
  __syncthreads();
  if (threadIdx.x < c && cnt[threadIdx.x] != 0) atomicAdd(&class_count[threadIdx.x], cnt[threadIdx.x]);
}

// C <= LR_CP: the row in registers (loss_rows.h); exp(x - m) is evaluated once per class instead of twice (the same call on the same
// operands: the same value)
template <typename T, int VB>
__global__ void __launch_bounds__(LV_THREADS)
lovasz_keys_rows_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target, int64_t n, int c,
                        int64_t ignore_index, int64_t* __restrict__ keys, int32_t* __restrict__ class_count) {
  __shared__ int32_t cnt[LV_MAX_C];
  if (threadIdx.x < LV_MAX_C) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (i < n) {
    float v[LR_CP];
    lr_load_row<T, VB>(logits + i * row_stride, c, v);
    const int64_t t = target[i];
    const bool valid = t != ignore_index && t >= 0 && t < c;
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < LR_CP; ++j) if (j < c) m = fmaxf(m, v[j]);
    float ssum = 0.f;
#pragma unroll
    for (int j = 0; j < LR_CP; ++j) if (j < c) { v[j] = __expf(v[j] - m); ssum += v[j]; }
    const float inv = 1.f / ssum;
#pragma unroll
    for (int j = 0; j < LR_CP; ++j) {
      if (j < c) {
        const float p = v[j] * inv;
        float e = valid ? (j == t ? 1.f - p : p) : 0.f;
        e = fminf(fmaxf(e, 0.f), 1.f);
        keys[(int64_t)j * n + i] = lv_key(e, valid && j == t);
      }
    }
    if (valid) atomicAdd(&cnt[(int)t], 1);
  }
  __syncthreads();
  if (threadIdx.x < c && cnt[threadIdx.x] != 0) atomicAdd(&class_count[threadIdx.x], cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(LV_THREADS)
lovasz_fg_kernel(const int64_t* __restrict__ sorted_keys, int64_t total, int32_t* __restrict__ fg) {
  const int64_t t = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (t < total) fg[t] = (int32_t)(sorted_keys[t] & 1);
}

// one slot of lovasz_step: Jaccard step, the slot's share of the loss, the gradient w.r.t. the probability scattered back to the point.
// ONE fp64 division per slot: the two branches of ptc_lovasz_step (voxel_keys.h) share it through selects of numerator and denominator
// (same operands, same quotient), and the 1 / n_present of the gradient is a multiplication by the reciprocal the workgroup computed once.
__device__ __forceinline__ double lv_step_slot(int64_t key, int32_t src, int32_t cum_fg_excl, int32_t i, int32_t gts, double inv_present,
                                               float* __restrict__ gprob_row) {
  const int f = (int)(key & 1);
  const int32_t cum_fg = cum_fg_excl + f;              // inclusive
  const int32_t cum_bg = (i + 1) - cum_fg;
  const double U = (double)gts + (double)cum_bg, I = (double)(gts - cum_fg);
  const double step = (f ? 1.0 : I) / (f ? U : U * (U - 1.0));   // exact Jaccard difference, ptc_lovasz_step's two quotients
  const float e = lv_key_error(key);
  float g = (float)(step * inv_present);
  g = f ? -g : g;                                      // d|fg - p| / dp
  gprob_row[src] = g;
  return (double)e * step;
}

// grid (G, c): class row blockIdx.y, G workgroups stride over its n sorted slots.  The first form of this kernel was ONE flat grid over the
// c n slots: `row = t / n` is a 64-bit integer division per slot (a ~100-instruction software sequence) and the step took three fp64 divisions
// (both Jaccard branches + step / n_present): 338 us at 819200 x 20 for 460 MB of streams -- compute, not the 4-byte scatter, bound it
// (profiles/r05_s_lovasz_xcd_rows.txt had already shown that the write-backs do not).  Rows with no foreground (gts == 0: class absent) give
// zero gradient and contribute nothing.
__global__ void __launch_bounds__(LV_THREADS)
lovasz_step_kernel(const int64_t* __restrict__ sorted_keys, const int64_t* __restrict__ order,
                   const int64_t* __restrict__ fg_scan, const int32_t* __restrict__ class_count, int64_t n, int c,
                   float* __restrict__ gprob, double* __restrict__ partial) {
  __shared__ double red[LV_THREADS / 64];
  __shared__ int n_present_s;
  if (threadIdx.x == 0) {
    int np = 0;
    for (int j = 0; j < c; ++j) np += class_count[j] > 0 ? 1 : 0;
    n_present_s = np;
  }
  __syncthreads();
  const double inv_present = 1.0 / (double)n_present_s;
  const int row = (int)blockIdx.y;
  const int64_t base = (int64_t)row * n;
  const int32_t gts = class_count[row], nn = (int32_t)n;
  const int64_t* __restrict__ kr = sorted_keys + base;
  const int64_t* __restrict__ orr = order + base;
  const int64_t* __restrict__ sr = fg_scan + base;
  float* __restrict__ gr = gprob + base;
  double contrib = 0.0;
  if (gts > 0) {
    const int64_t scan0 = sr[0];
    for (int32_t i = (int32_t)(blockIdx.x * LV_THREADS + threadIdx.x); i < nn; i += (int32_t)(gridDim.x * LV_THREADS))
      contrib += lv_step_slot(kr[i], (int32_t)orr[i], (int32_t)(sr[i] - scan0), i, gts, inv_present, gr);
  } else {
    for (int32_t i = (int32_t)(blockIdx.x * LV_THREADS + threadIdx.x); i < nn; i += (int32_t)(gridDim.x * LV_THREADS)) gr[i] = 0.f;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) contrib += __shfl_xor(contrib, o, 64);
  if (ptc_lane() == 0) red[threadIdx.x >> 6] = contrib;
  __syncthreads();
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(LV_THREADS)
lovasz_finish_kernel(const double* __restrict__ partial, int64_t n_partial, const int32_t* __restrict__ class_count, int c,
                     float* __restrict__ loss) {
  __shared__ double red[LV_THREADS];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n_partial; i += LV_THREADS) acc += partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = LV_THREADS / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int np = 0;
    for (int j = 0; j < c; ++j) np += class_count[j] > 0 ? 1 : 0;
    loss[0] = np > 0 ? (float)(red[0] / (double)np) : 0.f;
  }
}

template <typename T>
__global__ void __launch_bounds__(LV_THREADS)
lovasz_dlogits_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target,
                      const float* __restrict__ gprob, int64_t n, int c, int64_t ignore_index, float* __restrict__ dlogits) {
  const int64_t i = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (i >= n) return;
  const T* row = logits + i * row_stride;
  float* drow = dlogits + i * (int64_t)c;
  const int64_t t = target[i];
  const bool valid = t != ignore_index && t >= 0 && t < c;
  if (!valid) {
    for (int j = 0; j < c; ++j) drow[j] = 0.f;
    return;
  }
  float m = -INFINITY;
  for (int j = 0; j < c; ++j) m = fmaxf(m, ptc_to_float(row[j]));
  float ssum = 0.f;
  for (int j = 0; j < c; ++j) ssum += __expf(ptc_to_float(row[j]) - m);
  const float inv = 1.f / ssum;
  float dot = 0.f;
  for (int j = 0; j < c; ++j) dot += gprob[(int64_t)j * n + i] * (__expf(ptc_to_float(row[j]) - m) * inv);
  for (int j = 0; j < c; ++j) {
    const float p = __expf(ptc_to_float(row[j]) - m) * inv;
    drow[j] = p * (gprob[(int64_t)j * n + i] - dot);
  }
}

// C <= LR_CP: row in registers, the gradient rows out through LDS (loss_rows.h); the arithmetic is lovasz_dlogits_kernel's
template <typename T, int VB>
__global__ void __launch_bounds__(LV_THREADS)
lovasz_dlogits_rows_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target,
                           const float* __restrict__ gprob, int64_t n, int c, int64_t ignore_index, float* __restrict__ dlogits, int a16) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // [256][c] fp32: this workgroup's chunk of dlogits
  const int64_t row0 = (int64_t)blockIdx.x * LV_THREADS, i = row0 + threadIdx.x;
  if (i < n) {
    float* drow = reinterpret_cast<float*>(smem) + (int)threadIdx.x * c;
    const int64_t t = target[i];
    const bool valid = t != ignore_index && t >= 0 && t < c;
    if (!valid) {
#pragma unroll
      for (int j = 0; j < LR_CP; ++j) if (j < c) drow[j] = 0.f;
    } else {
      float v[LR_CP], gp[LR_CP];
      lr_load_row<T, VB>(logits + i * row_stride, c, v);
#pragma unroll
      for (int j = 0; j < LR_CP; ++j) gp[j] = j < c ? gprob[(int64_t)j * n + i] : 0.f;
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < LR_CP; ++j) if (j < c) m = fmaxf(m, v[j]);
      float ssum = 0.f;
#pragma unroll
      for (int j = 0; j < LR_CP; ++j) if (j < c) { v[j] = __expf(v[j] - m); ssum += v[j]; }
      const float inv = 1.f / ssum;
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < LR_CP; ++j) if (j < c) dot += gp[j] * (v[j] * inv);
#pragma unroll
      for (int j = 0; j < LR_CP; ++j) {
        if (j < c) {
          const float p = v[j] * inv;
          drow[j] = p * (gp[j] - dot);
        }
      }
    }
  }
  __syncthreads();
  const int64_t rows = (n - row0) < LV_THREADS ? (n - row0) : LV_THREADS;
  lr_copy_out<float>(smem, dlogits + row0 * c, (int)rows * c, a16 != 0);
}

struct LvLayout {
  size_t keys, order, fg, scan, gprob, partial, count, sort_ws, scan_ws, total;
  int64_t n_partial;
};
static LvLayout lv_layout(int64_t n, int c) {
  LvLayout L;
  const size_t nc = (size_t)(n > 0 ? n : 1) * (size_t)c;
  int64_t g = ptc_cdiv(n > 0 ? n : 1, LV_THREADS);           // lovasz_step: G workgroups per class row, one partial each
  if (g > LV_STEP_BLOCKS / c) g = LV_STEP_BLOCKS / c;
  L.n_partial = (g > 0 ? g : 1) * c;
  size_t o = 0;
  L.keys = o; o += ptc_align_up(nc * 8, 256);
  L.order = o; o += ptc_align_up(nc * 8, 256);
  L.fg = o; o += ptc_align_up(nc * 4, 256);
  L.scan = o; o += ptc_align_up(nc * 8, 256);
  L.gprob = o; o += ptc_align_up(nc * 4, 256);
  L.partial = o; o += ptc_align_up((size_t)L.n_partial * 8, 256);
  L.count = o; o += 256;
  L.sort_ws = o; o += ptc_align_up(ptc_sort_keys_workspace_bytes(n, c), 256);
  L.scan_ws = o; o += ptc_align_up(ptc_exclusive_scan_workspace_bytes((int64_t)nc), 256);
  L.total = o;
  return L;
}

extern "C" size_t ptc_lovasz_softmax_workspace_bytes(int64_t n, int c) {
  if (n < 0 || c < 1 || c > LV_MAX_C) return 0;
  return lv_layout(n, c).total;
}

extern "C" int ptc_lovasz_softmax(const void* logits, int64_t row_stride, const int64_t* target, int64_t n, int c, int dtype,
                                  int64_t ignore_index, float* loss, float* dlogits, void* workspace,
                                  size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && c >= 1 && row_stride >= c, PTC_EINVAL, "ptc_lovasz_softmax: bad sizes");
  PTC_REQUIRE(c <= LV_MAX_C, PTC_EUNSUPPORTED, "ptc_lovasz_softmax: c=%d > %d classes", c, LV_MAX_C);
  PTC_REQUIRE(n < (1ll << 31), PTC_EUNSUPPORTED, "ptc_lovasz_softmax: n >= 2^31");
  PTC_REQUIRE(loss != nullptr, PTC_EINVAL, "ptc_lovasz_softmax: null loss");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    PTC_HIP(hipMemsetAsync(loss, 0, sizeof(float), s));
    return PTC_OK;
  }
  PTC_REQUIRE(logits && target && dlogits && workspace, PTC_EINVAL, "ptc_lovasz_softmax: null buffer");
  const LvLayout L = lv_layout(n, c);
  PTC_REQUIRE(workspace_bytes >= L.total, PTC_EWORKSPACE, "ptc_lovasz_softmax: workspace %zu < %zu", workspace_bytes, L.total);
  char* ws = (char*)workspace;
  int64_t* keys = (int64_t*)(ws + L.keys);
  int64_t* order = (int64_t*)(ws + L.order);
  int32_t* fg = (int32_t*)(ws + L.fg);
  int64_t* scan = (int64_t*)(ws + L.scan);
  float* gprob = (float*)(ws + L.gprob);
  double* partial = (double*)(ws + L.partial);
  int32_t* count = (int32_t*)(ws + L.count);
  const int64_t nc = n * (int64_t)c;
  const unsigned grid_n = (unsigned)ptc_cdiv(n, LV_THREADS), grid_nc = (unsigned)ptc_cdiv(nc, LV_THREADS);

  const bool rows = c <= LR_CP;                      // the row-in-registers kernels (loss_rows.h)
  const int vb = lr_vec_bytes(logits, row_stride, c, ptc_dtype_size(dtype));
  PTC_HIP(hipMemsetAsync(count, 0, 256, s));
  if (rows) {
    PTC_DISPATCH_DTYPE(dtype, T, LR_DISPATCH_VB(vb, VB, hipLaunchKernelGGL((lovasz_keys_rows_kernel<T, VB>), dim3(grid_n), dim3(LV_THREADS), 0, s,
                                                                         (const T*)logits, row_stride, target, n, c, ignore_index, keys, count)))
  } else {
    PTC_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(lovasz_keys_kernel<T>, dim3(grid_n), dim3(LV_THREADS), 0, s, (const T*)logits,
                                                     row_stride, target, n, c, ignore_index, keys, count))
  }
  PTC_CHECK_LAUNCH("lovasz_keys_kernel");
  // the sorted key words replace the unsorted ones in place (the sort reads `keys` in its first pass only)
  int rc = ptc_sort_keys_ex(keys, n, c, 1, 31, order, nullptr, keys, ws + L.sort_ws, L.scan_ws - L.sort_ws, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(lovasz_fg_kernel, dim3(grid_nc), dim3(LV_THREADS), 0, s, keys, nc, fg);
  PTC_CHECK_LAUNCH("lovasz_fg_kernel");
  rc = ptc_exclusive_scan_i32(fg, nc, scan, ws + L.scan_ws, L.total - L.scan_ws, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(lovasz_step_kernel, dim3((unsigned)(L.n_partial / c), (unsigned)c), dim3(LV_THREADS), 0, s, keys, order, scan, count, n, c, gprob,
                     partial);
  PTC_CHECK_LAUNCH("lovasz_step_kernel");
  hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(LV_THREADS), 0, s, partial, L.n_partial, count, c, loss);
  PTC_CHECK_LAUNCH("lovasz_finish_kernel");
  if (rows) {
    const int a16 = ((uintptr_t)dlogits & 15) == 0;
    const size_t lds = (size_t)LV_THREADS * c * sizeof(float);
    PTC_DISPATCH_DTYPE(dtype, T, LR_DISPATCH_VB(vb, VB, hipLaunchKernelGGL((lovasz_dlogits_rows_kernel<T, VB>), dim3(grid_n), dim3(LV_THREADS), lds, s,
                                                                         (const T*)logits, row_stride, target, gprob, n, c, ignore_index, dlogits,
                                                                         a16)))
  } else {
    PTC_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(lovasz_dlogits_kernel<T>, dim3(grid_n), dim3(LV_THREADS), 0, s, (const T*)logits,
                                                     row_stride, target, gprob, n, c, ignore_index, dlogits))
  }
  PTC_CHECK_LAUNCH("lovasz_dlogits_kernel");
  return PTC_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// Row-compacted path, 1 <= c <= LW_MAX_C (ScanNet200: 200 classes, ScanNet++: 100).  The reference sorts only the classes labels.unique()
// returns; a class without a counted point has zero loss and zero probability gradient, so its row of the [c, n] error matrix never
// exists here: the P present classes get the compact rows 0..P-1 in ascending class order (ptc_lovasz_present), and keys, sort, scan,
// steps and gprob are [P, n] -- ~56 B per slot of workspace where the dense layout above would take 9 GB at 819200 x 200.
//   lovasz_count / lovasz_rank  : class populations (LDS histogram, integer atomics) and the ranking of the present classes
//   lovasz_keys_wide            : a workgroup owns a tile of consecutive points; a group of lanes reads one logits row with the widest
//                                 loads its alignment allows, softmax ONCE per row in fp32 (the row in registers, group reductions),
//                                 probabilities into an LDS tile [points][classes]; then every present class takes its column of the
//                                 tile: keys[row * n + i] in runs of consecutive points.  Absent classes write nothing.
//   sort / fg / scan            : as above, over P rows
//   lovasz_step_rows / _finish_rows : lv_step_slot per slot; gts = class_count[class_of[row]], 1 / P from n_present
//   lovasz_dlogits_wide         : the same tile and softmax; gprob's compact rows gathered into a second tile (zero where a class is
//                                 absent); dz = p * (g - <g, p>) written row after row (contiguous), zeros for uncounted points.
// The tile's point count shrinks as c grows (LW_TILE_BYTES per tile: 64 points up to 120 classes, 32 up to 248, 16 up to 504, 8 up to 1016) instead of
// the class axis being cut into chunks: a chunked class axis needs the row's maximum and sum before its first chunk's probabilities,
// i.e. a second evaluation of every exp.
#define LW_MAX_C PTC_LOVASZ_MAX_C
#define LW_RV 16                       // registers of one lane holding its share of a row: 64 lanes x 16 = 1024 classes
#define LW_TILE_BYTES (32 * 1024)         // two images (dlogits) stay inside the 64 KB a launch gets without opting in

__global__ void __launch_bounds__(LV_THREADS)
lovasz_count_kernel(const int64_t* __restrict__ target, int64_t n, int c, int64_t ignore_index, int32_t* __restrict__ class_count) {
  __shared__ int32_t cnt[LW_MAX_C];
  for (int j = threadIdx.x; j < c; j += LV_THREADS) cnt[j] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * LV_THREADS) {
    const int64_t t = target[i];
    if (t != ignore_index && t >= 0 && t < c) atomicAdd(&cnt[(int)t], 1);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < c; j += LV_THREADS)
    if (cnt[j] != 0) atomicAdd(&class_count[j], cnt[j]);
}

// one workgroup: thread t ranks the classes [4t, 4t + 4) -- exclusive scan of the presence flags in ascending class order
__global__ void __launch_bounds__(LV_THREADS)
lovasz_rank_kernel(const int32_t* __restrict__ class_count, int c, int32_t* __restrict__ row_of, int32_t* __restrict__ class_of,
                   int32_t* __restrict__ n_present) {
  __shared__ int32_t wsum[LV_THREADS / 64];
  constexpr int PER = LW_MAX_C / LV_THREADS;
  const int lane = ptc_lane(), wave = threadIdx.x >> 6, j0 = (int)threadIdx.x * PER;
  bool f[PER];
  int32_t mine = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    f[q] = j0 + q < c && class_count[j0 + q] > 0;
    mine += f[q] ? 1 : 0;
  }
  int32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int32_t before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < LV_THREADS / 64; ++w) {
    before += w < wave ? wsum[w] : 0;
    total += wsum[w];
  }
  int32_t r = before + incl - mine;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int j = j0 + q;
    if (j < c) {
      row_of[j] = f[q] ? r : -1;
      if (f[q]) class_of[r++] = j;
    }
  }
  for (int k = total + (int)threadIdx.x; k < c; k += LV_THREADS) class_of[k] = -1;
  if (threadIdx.x == 0) n_present[0] = total;
}

extern "C" int ptc_lovasz_present(const int64_t* target, int64_t n, int c, int64_t ignore_index, int32_t* class_count, int32_t* row_of,
                                  int32_t* class_of, int32_t* n_present, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && c >= 1, PTC_EINVAL, "ptc_lovasz_present: bad sizes");
  PTC_REQUIRE(c <= LW_MAX_C, PTC_EUNSUPPORTED, "ptc_lovasz_present: c=%d > %d classes", c, LW_MAX_C);
  PTC_REQUIRE(n < (1ll << 31), PTC_EUNSUPPORTED, "ptc_lovasz_present: n >= 2^31");
  PTC_REQUIRE(class_count && row_of && class_of && n_present && (target || n == 0), PTC_EINVAL, "ptc_lovasz_present: null buffer");
  hipStream_t s = (hipStream_t)stream;
  PTC_HIP(hipMemsetAsync(class_count, 0, (size_t)c * sizeof(int32_t), s));
  if (n > 0) {
    int64_t grid = ptc_cdiv(n, LV_THREADS * 4);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(lovasz_count_kernel, dim3((unsigned)grid), dim3(LV_THREADS), 0, s, target, n, c, ignore_index, class_count);
    PTC_CHECK_LAUNCH("lovasz_count_kernel");
  }
  hipLaunchKernelGGL(lovasz_rank_kernel, dim3(1), dim3(LV_THREADS), 0, s, class_count, c, row_of, class_of, n_present);
  PTC_CHECK_LAUNCH("lovasz_rank_kernel");
  return PTC_OK;
}

// Softmax of the tile's counted points into `tile` [tp][ld] fp32 and their labels (-1 = not counted) into tgt_s [tp].  2^gl_log2 lanes
// share a row: lane l of the group holds the classes [(q * group + l) * E, + E) of pass q in registers -- one vector load each, E = the
// elements of the widest load the rows' alignment allows (lr_vec_bytes).  Classes past c hold -inf: exp gives them 0.  The same
// __expf(x - m) * inv as lovasz_keys_kernel, every exp evaluated once.  Rows of uncounted points are left untouched (nobody reads them).
// Every shuffle is met by the whole wave: the loops' trip counts are workgroup-uniform, only loads and stores are predicated.
template <typename T, int VB>
__device__ __forceinline__ void lw_softmax_tile(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target, int64_t n,
                                                int c, int64_t ignore_index, int64_t i0, int tp, int ld, int gl_log2,
                                                float* __restrict__ tile, int32_t* __restrict__ tgt_s) {
  constexpr int E = VB == 0 ? 1 : VB / (int)sizeof(T);
  constexpr int NQ = LW_RV / E;
  const int gl = 1 << gl_log2, l = ptc_lane() & (gl - 1);
  for (int r0 = 0; r0 < tp; r0 += LV_THREADS >> gl_log2) {
    const int r = r0 + ((int)threadIdx.x >> gl_log2);
    const int64_t i = i0 + r;
    int32_t t = -1;
    if (r < tp && i < n) {
      const int64_t t64 = target[i];
      if (t64 != ignore_index && t64 >= 0 && t64 < c) t = (int32_t)t64;
    }
    if (r < tp && l == 0) tgt_s[r] = t;
    const bool live = t >= 0;
    const T* row = logits + i * row_stride;
    float v[LW_RV];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q * gl * E < c) {
        const int j = (q * gl + l) * E;
        if (live && j < c) {
          if constexpr (VB == 0) {
            v[q] = ptc_to_float(row[j]);
          } else {
            __attribute__((aligned(16))) T tmp[E];
            if constexpr (VB == 16) *reinterpret_cast<uint4*>(tmp) = *reinterpret_cast<const uint4*>(row + j);
            else *reinterpret_cast<uint2*>(tmp) = *reinterpret_cast<const uint2*>(row + j);
#pragma unroll
            for (int e = 0; e < E; ++e) v[q * E + e] = j + e < c ? ptc_to_float(tmp[e]) : -INFINITY;
          }
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e) v[q * E + e] = -INFINITY;
        }
      }
    }
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q * gl * E < c) {
#pragma unroll
        for (int e = 0; e < E; ++e) m = fmaxf(m, v[q * E + e]);
      }
    }
    for (int o = gl >> 1; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float ssum = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q * gl * E < c) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          v[q * E + e] = __expf(v[q * E + e] - m);
          ssum += v[q * E + e];
        }
      }
    }
    for (int o = gl >> 1; o >= 1; o >>= 1) ssum += __shfl_xor(ssum, o, 64);
    const float inv = 1.f / ssum;
    if (live) {
      float* prow = tile + r * ld;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = (q * gl + l) * E;
        if (q * gl * E < c && j < c) {
          if constexpr (E >= 4) {
#pragma unroll
            for (int e = 0; e < E; e += 4)
              *reinterpret_cast<float4*>(prow + j + e) = make_float4(v[q * E + e] * inv, v[q * E + e + 1] * inv, v[q * E + e + 2] * inv,
                                                                      v[q * E + e + 3] * inv);
          } else if constexpr (E == 2) {
            *reinterpret_cast<float2*>(prow + j) = make_float2(v[q * E] * inv, v[q * E + 1] * inv);
          } else {
            prow[j] = v[q] * inv;
          }
        }
      }
    }
  }
}

// grid = tiles of tp = 2^tp_log2 points; dynamic LDS = tile [tp][ld] fp32 + labels [tp] int32
template <typename T, int VB>
__global__ void __launch_bounds__(LV_THREADS)
lovasz_keys_wide_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target, int64_t n, int c,
                        int64_t ignore_index, const int32_t* __restrict__ class_of, const int32_t* __restrict__ n_present, int rows,
                        int tp_log2, int ld, int gl_log2, int64_t* __restrict__ keys) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tp = 1 << tp_log2;
  float* tile = reinterpret_cast<float*>(smem);
  int32_t* tgt_s = reinterpret_cast<int32_t*>(smem + (size_t)tp * ld * sizeof(float));
  const int64_t i0 = (int64_t)blockIdx.x * tp;
  lw_softmax_tile<T, VB>(logits, row_stride, target, n, c, ignore_index, i0, tp, ld, gl_log2, tile, tgt_s);
  __syncthreads();
  const int np = n_present[0] < rows ? n_present[0] : rows;     // `rows` sized the workspace
  const int i = (int)threadIdx.x & (tp - 1);
  const int64_t gi = i0 + i;
  if (gi >= n) return;
  const int32_t t = tgt_s[i];
  for (int r = (int)threadIdx.x >> tp_log2; r < np; r += LV_THREADS >> tp_log2) {
    const int j = class_of[r];
    const bool fg = j == t;
    float e = 0.f;
    if (t >= 0) {
      const float p = tile[i * ld + j];
      e = fg ? 1.f - p : p;
    }
    e = fminf(fmaxf(e, 0.f), 1.f);
    keys[(int64_t)r * n + gi] = lv_key(e, fg);
  }
}

// lovasz_step_kernel over the P compact rows: the same slots (lv_step_slot), gts = the population of the row's class, 1 / P from n_present
__global__ void __launch_bounds__(LV_THREADS)
lovasz_step_rows_kernel(const int64_t* __restrict__ sorted_keys, const int64_t* __restrict__ order, const int64_t* __restrict__ fg_scan,
                        const int32_t* __restrict__ class_count, const int32_t* __restrict__ class_of, const int32_t* __restrict__ n_present,
                        int64_t n, float* __restrict__ gprob, double* __restrict__ partial) {
  __shared__ double red[LV_THREADS / 64];
  const int row = (int)blockIdx.y, np = n_present[0];
  double contrib = 0.0;
  if (row < np) {
    const double inv_present = 1.0 / (double)np;
    const int64_t base = (int64_t)row * n;
    const int32_t gts = class_count[class_of[row]], nn = (int32_t)n;
    const int64_t* __restrict__ kr = sorted_keys + base;
    const int64_t* __restrict__ orr = order + base;
    const int64_t* __restrict__ sr = fg_scan + base;
    float* __restrict__ gr = gprob + base;
    const int64_t scan0 = sr[0];
    for (int32_t i = (int32_t)(blockIdx.x * LV_THREADS + threadIdx.x); i < nn; i += (int32_t)(gridDim.x * LV_THREADS))
      contrib += lv_step_slot(kr[i], (int32_t)orr[i], (int32_t)(sr[i] - scan0), i, gts, inv_present, gr);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) contrib += __shfl_xor(contrib, o, 64);
  if (ptc_lane() == 0) red[threadIdx.x >> 6] = contrib;
  __syncthreads();
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(LV_THREADS)
lovasz_finish_rows_kernel(const double* __restrict__ partial, int64_t n_partial, const int32_t* __restrict__ n_present, float* __restrict__ loss) {
  __shared__ double red[LV_THREADS];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n_partial; i += LV_THREADS) acc += partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = LV_THREADS / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int np = n_present[0];
    loss[0] = np > 0 ? (float)(red[0] / (double)np) : 0.f;
  }
}

// dynamic LDS = probabilities [tp][ld] + gprob [tp][ld] (fp32) + labels [tp]; 2^g3_log2 lanes write one dlogits row
template <typename T, int VB>
__global__ void __launch_bounds__(LV_THREADS)
lovasz_dlogits_wide_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target, int64_t n, int c,
                           int64_t ignore_index, const int32_t* __restrict__ class_of, const int32_t* __restrict__ n_present, int rows,
                           const float* __restrict__ gprob, int tp_log2, int ld, int gl_log2, int g3_log2, float* __restrict__ dlogits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tp = 1 << tp_log2;
  float* tile = reinterpret_cast<float*>(smem);
  float* gt = tile + tp * ld;
  int32_t* tgt_s = reinterpret_cast<int32_t*>(gt + tp * ld);
  const int64_t i0 = (int64_t)blockIdx.x * tp;
  for (int k = threadIdx.x; k < tp * ld / 4; k += LV_THREADS) reinterpret_cast<float4*>(gt)[k] = make_float4(0.f, 0.f, 0.f, 0.f);   // absent: g = 0
  lw_softmax_tile<T, VB>(logits, row_stride, target, n, c, ignore_index, i0, tp, ld, gl_log2, tile, tgt_s);
  __syncthreads();
  {
    const int np = n_present[0] < rows ? n_present[0] : rows;
    const int i = (int)threadIdx.x & (tp - 1);
    const int64_t gi = i0 + i;
    if (gi < n && tgt_s[i] >= 0)
      for (int r = (int)threadIdx.x >> tp_log2; r < np; r += LV_THREADS >> tp_log2) gt[i * ld + class_of[r]] = gprob[(int64_t)r * n + gi];
  }
  __syncthreads();
  const int g3 = 1 << g3_log2, l = ptc_lane() & (g3 - 1);
  for (int r0 = 0; r0 < tp; r0 += LV_THREADS >> g3_log2) {
    const int r = r0 + ((int)threadIdx.x >> g3_log2);
    const int64_t i = i0 + r;
    const bool inside = r < tp && i < n, counted = inside && tgt_s[r] >= 0;
    const float* prow = tile + r * ld;
    const float* grow = gt + r * ld;
    float dot = 0.f;
    if (counted)
      for (int j = l; j < c; j += g3) dot += grow[j] * prow[j];
    for (int o = g3 >> 1; o >= 1; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if (inside) {
      float* drow = dlogits + i * (int64_t)c;
      for (int j = l; j < c; j += g3) drow[j] = counted ? prow[j] * (grow[j] - dot) : 0.f;
    }
  }
}

static int lw_ld(int c) { return (c + 7) / 8 * 8 + 4; }      // a multiple of 4 (16-byte rows), 4 * odd: columns of 8 rows meet 8 different banks
static size_t lw_lds_bytes(int c, int tiles, int tp_log2) {
  return (size_t)tiles * (1 << tp_log2) * lw_ld(c) * sizeof(float) + (size_t)(1 << tp_log2) * sizeof(int32_t);
}
// points per tile: the largest power of two in [4, 64] whose `tiles` fp32 images and labels fit LW_TILE_BYTES per image
static int lw_tp_log2(int c, int tiles) {
  int l = 6;
  while (l > 2 && lw_lds_bytes(c, tiles, l) > (size_t)tiles * LW_TILE_BYTES) --l;
  return l;
}
// lanes per row: the smallest power of two (at most a wave) that covers c with one e-element piece per lane
static int lw_group_log2(int c, int e) {
  int l = 0;
  while (l < 6 && (1 << l) * e < c) ++l;
  return l;
}

extern "C" size_t ptc_lovasz_softmax_rows_workspace_bytes(int64_t n, int c, int rows) {
  if (n < 0 || c < 1 || c > LW_MAX_C || rows < 0 || rows > c) return 0;
  if (n == 0 || rows == 0) return 0;
  return lv_layout(n, rows).total;
}

extern "C" int ptc_lovasz_softmax_rows(const void* logits, int64_t row_stride, const int64_t* target, int64_t n, int c, int dtype,
                                       int64_t ignore_index, const int32_t* class_count, const int32_t* row_of, const int32_t* class_of,
                                       const int32_t* n_present, int rows, float* loss, float* dlogits, void* workspace,
                                       size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && c >= 1 && row_stride >= c, PTC_EINVAL, "ptc_lovasz_softmax_rows: bad sizes");
  PTC_REQUIRE(c <= LW_MAX_C, PTC_EUNSUPPORTED, "ptc_lovasz_softmax_rows: c=%d > %d classes", c, LW_MAX_C);
  PTC_REQUIRE(n < (1ll << 31), PTC_EUNSUPPORTED, "ptc_lovasz_softmax_rows: n >= 2^31");
  PTC_REQUIRE(rows >= 0 && rows <= c, PTC_EINVAL, "ptc_lovasz_softmax_rows: rows=%d outside [0, %d]", rows, c);
  PTC_REQUIRE(loss != nullptr, PTC_EINVAL, "ptc_lovasz_softmax_rows: null loss");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0 || rows == 0) {                       // nothing counted: loss 0, zero gradient
    PTC_HIP(hipMemsetAsync(loss, 0, sizeof(float), s));
    if (n > 0) {
      PTC_REQUIRE(dlogits != nullptr, PTC_EINVAL, "ptc_lovasz_softmax_rows: null dlogits");
      PTC_HIP(hipMemsetAsync(dlogits, 0, (size_t)n * c * sizeof(float), s));
    }
    return PTC_OK;
  }
  PTC_REQUIRE(logits && target && dlogits && workspace && class_count && row_of && class_of && n_present, PTC_EINVAL,
              "ptc_lovasz_softmax_rows: null buffer");
  const LvLayout L = lv_layout(n, rows);
  PTC_REQUIRE(workspace_bytes >= L.total, PTC_EWORKSPACE, "ptc_lovasz_softmax_rows: workspace %zu < %zu", workspace_bytes, L.total);
  char* ws = (char*)workspace;
  int64_t* keys = (int64_t*)(ws + L.keys);
  int64_t* order = (int64_t*)(ws + L.order);
  int32_t* fg = (int32_t*)(ws + L.fg);
  int64_t* scan = (int64_t*)(ws + L.scan);
  float* gprob = (float*)(ws + L.gprob);
  double* partial = (double*)(ws + L.partial);
  const int64_t nr = n * (int64_t)rows;
  const int vb = lr_vec_bytes(logits, row_stride, c, ptc_dtype_size(dtype));
  const int elems = vb == 0 ? 1 : vb / (int)ptc_dtype_size(dtype);
  const int gl = lw_group_log2(c, elems), g3 = lw_group_log2(c, 1), ld = lw_ld(c);

  const int tpk = lw_tp_log2(c, 1);
  PTC_DISPATCH_DTYPE(dtype, T, LR_DISPATCH_VB(vb, VB, hipLaunchKernelGGL((lovasz_keys_wide_kernel<T, VB>), dim3((unsigned)ptc_cdiv(n, 1 << tpk)),
                                                                       dim3(LV_THREADS), lw_lds_bytes(c, 1, tpk), s, (const T*)logits, row_stride,
                                                                       target, n, c, ignore_index, class_of, n_present, rows, tpk, ld, gl, keys)))
  PTC_CHECK_LAUNCH("lovasz_keys_wide_kernel");
  int rc = ptc_sort_keys_ex(keys, n, rows, 1, 31, order, nullptr, keys, ws + L.sort_ws, L.scan_ws - L.sort_ws, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(lovasz_fg_kernel, dim3((unsigned)ptc_cdiv(nr, LV_THREADS)), dim3(LV_THREADS), 0, s, keys, nr, fg);
  PTC_CHECK_LAUNCH("lovasz_fg_kernel");
  rc = ptc_exclusive_scan_i32(fg, nr, scan, ws + L.scan_ws, L.total - L.scan_ws, stream);
  if (rc != PTC_OK) return rc;
  hipLaunchKernelGGL(lovasz_step_rows_kernel, dim3((unsigned)(L.n_partial / rows), (unsigned)rows), dim3(LV_THREADS), 0, s, keys, order, scan,
                     class_count, class_of, n_present, n, gprob, partial);
  PTC_CHECK_LAUNCH("lovasz_step_rows_kernel");
  hipLaunchKernelGGL(lovasz_finish_rows_kernel, dim3(1), dim3(LV_THREADS), 0, s, partial, L.n_partial, n_present, loss);
  PTC_CHECK_LAUNCH("lovasz_finish_rows_kernel");
  const int tpd = lw_tp_log2(c, 2);
  PTC_DISPATCH_DTYPE(dtype, T, LR_DISPATCH_VB(vb, VB, hipLaunchKernelGGL((lovasz_dlogits_wide_kernel<T, VB>), dim3((unsigned)ptc_cdiv(n, 1 << tpd)),
                                                                       dim3(LV_THREADS), lw_lds_bytes(c, 2, tpd), s, (const T*)logits, row_stride,
                                                                       target, n, c, ignore_index, class_of, n_present, rows, gprob, tpd, ld, gl, g3,
                                                                       dlogits)))
  PTC_CHECK_LAUNCH("lovasz_dlogits_wide_kernel");
  return PTC_OK;
}
