// augment.hip -- the point augmentations of pointcept/datasets/transform.py for clouds that already live on the device: a run of affine
// transforms is ONE pending 3 x 4 matrix per scene (held on the device in double, never read by the host), coordinates are written
// once per flush.
//   state   aff [21] double = A [3x3] row-major, t [3], Rn [3x3]: coord' = A p + t, normal' = Rn n (Rn takes rotations and flips only,
//           as the reference treats normals: transform.py:279-280, :347-353).
//           stats [12] double = min xyz, max xyz of the cloud under the pending affine, then min rgb, max rgb of the colours.
//   ptc_aug_reduce         one read-only pass: per-workgroup partial min / max of A p + t and of the colour channels, then a finish over
//                          the partial rows.  min / max are exact and order-free: no atomics, bit-reproducible.
//   ptc_aug_compose        one thread advances (A, t, Rn) by a host-built list of op descriptors; CenterShift (:172-185) and a
//                          RandomRotate without a centre (:270-273) read the bounding box from `stats`, so the host reads nothing.  The
//                          box is carried exactly through shift / scale / flip (boxes map to boxes) and written back; a rotation does
//                          not map boxes to boxes, the caller reduces again before the next op that needs one.
//   ptc_aug_apply          the flush: coord' = A p + t (+ clip(sigma z, +-clip), RandomJitter :358-372) (clamped, PointClip :203-214),
//                          normal' = Rn n, the colour ops in their order (ChromaticAutoContrast :397-422, ChromaticTranslation :426-435,
//                          ChromaticJitter :439-451, NormalizeColor :143-147).  The affine is evaluated in double and rounded once.
//   ptc_aug_elastic_grid   ElasticDistortion's blurred noise grid (:793-812): two rounds of x, y, z box filters of width 3 with zero
//                          padding are Mx (x) My (x) Mz applied once, M[i][j] = #{k in [0, dim): |i-k| <= 1 and |k-j| <= 1} / 9.
//   ptc_aug_elastic_apply  per point p = A p0 + t, trilinear interpolation in the grid (origin min - g, spacing g, :815-826),
//                          p += interp * magnitude; writes the partial min / max of its output for the next stage.
//   noise   z(seed, stream, e): a counter-based standard normal (splitmix64 of the counter, Box-Muller), a pure function of its three
//           arguments -- independent of n and of the launch geometry.  Every consumer also takes an injected tensor instead.
// Nothing here synchronises or reads device memory from the host.
#include "ptc_common.h"
#include "ptcore_augment.h"
#include <math.h>

#define AU_THREADS 256
#define AU_PPT 4                              // points per thread
#define AU_TILE (AU_THREADS * AU_PPT)         // points per workgroup
#define AU_MAX_OPS PTC_AUG_MAX_OPS            // affine descriptors per compose launch (ptcore_augment.h)
#define AU_MAX_COLOR PTC_AUG_MAX_COLOR_OPS     // colour ops per flush
#define AU_FIN_SLOTS 16

enum { AU_CENTER_SHIFT = PTC_AUG_CENTER_SHIFT, AU_ROTATE = PTC_AUG_ROTATE, AU_SCALE = PTC_AUG_SCALE, AU_FLIP = PTC_AUG_FLIP, AU_SHIFT = PTC_AUG_SHIFT };
enum { AU_C_AUTOCONTRAST = PTC_AUG_C_AUTOCONTRAST, AU_C_TRANSLATION = PTC_AUG_C_TRANSLATION, AU_C_JITTER = PTC_AUG_C_JITTER,
       AU_C_NORMALIZE = PTC_AUG_C_NORMALIZE };

struct AuOps {
  int n;
  double v[AU_MAX_OPS][8];      // kind, then its arguments (ptcore_augment.h)
};

struct AuApply {
  const float *coord, *normal, *color;
  float *coord_out, *normal_out, *color_out;
  const double *aff, *stats;
  int64_t n;
  int jitter, pclip, ncolor;
  double sigma, jclip;
  const float* jnoise;
  uint64_t jseed;
  double range[6];
  int ckind[AU_MAX_COLOR], cstream[AU_MAX_COLOR];
  float cpar[AU_MAX_COLOR][3];
  const float* cnoise[AU_MAX_COLOR];
  uint64_t cseed[AU_MAX_COLOR];
};

// ---- the generator ------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t au_mix(uint64_t x) {      // splitmix64's output function
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
__host__ __device__ __forceinline__ uint64_t au_key(uint64_t seed, int stream) {
  return au_mix(seed ^ (0xD6E8FEB86659FD93ull * (uint64_t)(stream + 1)));
}
// element e of the stream with key k: two 24-bit uniforms in (0, 1] / (0, 1) from one 64-bit word, Box-Muller's cosine branch
__device__ __forceinline__ float au_normal(uint64_t k, uint64_t e) {
  const uint64_t h = au_mix(k + 0x9E3779B97F4A7C15ull * (e + 1));
  const float u1 = ((float)(uint32_t)(h >> 40) + 0.5f) * 5.9604644775390625e-8f;
  const float u2 = ((float)(uint32_t)((h >> 16) & 0xFFFFFFu) + 0.5f) * 5.9604644775390625e-8f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958648f * u2);
}

// ---- min / max of a workgroup -> one partial row ---------------------------------------------------------------------------------------
// lo[q], hi[q], q < NQ: the thread's own values; row: [2 * NQ] = lo..., hi...
template <int NQ>
__device__ __forceinline__ void au_block_minmax(double* lo, double* hi, double* __restrict__ row) {
  __shared__ double red[2 * NQ][AU_THREADS / 64];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      lo[q] = fmin(lo[q], __shfl_xor(lo[q], o, 64));
      hi[q] = fmax(hi[q], __shfl_xor(hi[q], o, 64));
    }
  }
  const int wave = threadIdx.x >> 6;
  if (ptc_lane() == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) { red[q][wave] = lo[q]; red[NQ + q][wave] = hi[q]; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * NQ) {
    const int q = threadIdx.x;
    double v = red[q][0];
#pragma unroll
    for (int w = 1; w < AU_THREADS / 64; ++w) v = q < NQ ? fmin(v, red[q][w]) : fmax(v, red[q][w]);
    row[q] = v;
  }
}

__device__ __forceinline__ void au_affine(const double* __restrict__ m, float x, float y, float z, double& ox, double& oy, double& oz) {
  ox = fma(m[0], (double)x, fma(m[1], (double)y, fma(m[2], (double)z, m[9])));
  oy = fma(m[3], (double)x, fma(m[4], (double)y, fma(m[5], (double)z, m[10])));
  oz = fma(m[6], (double)x, fma(m[7], (double)y, fma(m[8], (double)z, m[11])));
}

// partial [blocks, 12]: columns 0-5 coordinates (min xyz, max xyz), 6-11 colours
__global__ void __launch_bounds__(AU_THREADS)
aug_reduce_kernel(const float* __restrict__ coord, const float* __restrict__ color, int64_t n, const double* __restrict__ aff,
                  double* __restrict__ partial) {
  double lo[6], hi[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) { lo[q] = INFINITY; hi[q] = -INFINITY; }
  double m[12];
  if (aff) {
#pragma unroll
    for (int q = 0; q < 12; ++q) m[q] = aff[q];
  }
  for (int k = 0; k < AU_PPT; ++k) {
    const int64_t i = (int64_t)blockIdx.x * AU_TILE + k * AU_THREADS + threadIdx.x;
    if (i >= n) continue;
    if (coord) {
      const float x = coord[i * 3], y = coord[i * 3 + 1], z = coord[i * 3 + 2];
      double p[3] = {(double)x, (double)y, (double)z};
      if (aff) au_affine(m, x, y, z, p[0], p[1], p[2]);
#pragma unroll
      for (int q = 0; q < 3; ++q) { lo[q] = fmin(lo[q], p[q]); hi[q] = fmax(hi[q], p[q]); }
    }
    if (color) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double c = (double)color[i * 3 + q];
        lo[3 + q] = fmin(lo[3 + q], c);
        hi[3 + q] = fmax(hi[3 + q], c);
      }
    }
  }
  double* row = partial + (int64_t)blockIdx.x * 12;
  au_block_minmax<3>(lo, hi, row);
  __syncthreads();          // the helper's LDS is reused
  au_block_minmax<3>(lo + 3, hi + 3, row + 6);
}

// columns [first, first + w) of partial [rows, stride] -> stats[first + .]: triples alternate min, max.  One workgroup; min / max are
// exact, so any order gives the same bits.
__global__ void __launch_bounds__(AU_THREADS)
aug_finish_kernel(const double* __restrict__ partial, int64_t rows, int stride, int first, int w, double* __restrict__ stats) {
  __shared__ double red[12][AU_FIN_SLOTS];
  const int q = threadIdx.x / AU_FIN_SLOTS, s = threadIdx.x % AU_FIN_SLOTS;
  if (q < w) {
    const int c = first + q;
    const bool is_min = (c / 3) % 2 == 0;
    double v = is_min ? INFINITY : -INFINITY;
    for (int64_t r = s; r < rows; r += AU_FIN_SLOTS) v = is_min ? fmin(v, partial[r * stride + c]) : fmax(v, partial[r * stride + c]);
    red[q][s] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < w) {
    const int c = first + (int)threadIdx.x;
    const bool is_min = (c / 3) % 2 == 0;
    double v = red[threadIdx.x][0];
    for (int k = 1; k < AU_FIN_SLOTS; ++k) v = is_min ? fmin(v, red[threadIdx.x][k]) : fmax(v, red[threadIdx.x][k]);
    stats[c] = v;
  }
}

// ---- compose -----------------------------------------------------------------------------------------------------------------------------
// The rotation by (cs, sn) in the plane of the axes (I, J) = (y, z) | (z, x) | (x, y) about the centre c, applied on the left of the
// pending affine: rows I and J of A and Rn turn, t turns about c; the third row is the identity's (transform.py:260-278).  I and J
// are compile-time constants: every access is to a fixed element.  (A first form built a private 3 x 3 matrix under the axis branch and
// multiplied it in loops; compiled for gfx950 it rotated wrongly about z while the host emulation of the same source was right.)
template <int I, int J>
__device__ __forceinline__ void au_rotate(double cs, double sn, const double* c, double* A, double* t, double* Rn) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = A[I * 3 + k], b = A[J * 3 + k], na = Rn[I * 3 + k], nb = Rn[J * 3 + k];
    A[I * 3 + k] = cs * a - sn * b;
    A[J * 3 + k] = sn * a + cs * b;
    Rn[I * 3 + k] = cs * na - sn * nb;
    Rn[J * 3 + k] = sn * na + cs * nb;
  }
  const double ti = t[I] - c[I], tj = t[J] - c[J];
  t[I] = cs * ti - sn * tj + c[I];
  t[J] = sn * ti + cs * tj + c[J];
}

__global__ void __launch_bounds__(64)
aug_compose_kernel(AuOps ops, int from_identity, double* __restrict__ aff, double* __restrict__ stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, Rn[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (!from_identity) {
    for (int q = 0; q < 9; ++q) { A[q] = aff[q]; Rn[q] = aff[12 + q]; }
    for (int q = 0; q < 3; ++q) t[q] = aff[9 + q];
  }
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (stats) {
    for (int q = 0; q < 3; ++q) { lo[q] = stats[q]; hi[q] = stats[3 + q]; }
  }
  bool rotated = false;
  for (int o = 0; o < ops.n; ++o) {
    const double* v = ops.v[o];
    const int kind = (int)v[0];
    if (kind == AU_CENTER_SHIFT) {             // v[1]: apply_z
      const double d[3] = {-(lo[0] + hi[0]) / 2, -(lo[1] + hi[1]) / 2, v[1] != 0. ? -lo[2] : 0.};
      for (int q = 0; q < 3; ++q) { t[q] += d[q]; lo[q] += d[q]; hi[q] += d[q]; }
    } else if (kind == AU_ROTATE) {            // v[1]: axis 0 | 1 | 2, v[2] cos, v[3] sin, v[4]: centre given, v[5..8) the centre
      const double cs = v[2], sn = v[3];
      double c[3];
      for (int q = 0; q < 3; ++q) c[q] = v[4] != 0. ? v[5 + q] : (lo[q] + hi[q]) / 2;
      const int axis = (int)v[1];
      if (axis == 0) au_rotate<1, 2>(cs, sn, c, A, t, Rn);
      else if (axis == 1) au_rotate<2, 0>(cs, sn, c, A, t, Rn);
      else au_rotate<0, 1>(cs, sn, c, A, t, Rn);
      rotated = true;
    } else if (kind == AU_SCALE) {             // v[1..4)
      for (int r = 0; r < 3; ++r) {
        const double s = v[1 + r];
        for (int k = 0; k < 3; ++k) A[r * 3 + k] *= s;
        t[r] *= s;
        const double a = lo[r] * s, b = hi[r] * s;
        lo[r] = fmin(a, b);
        hi[r] = fmax(a, b);
      }
    } else if (kind == AU_FLIP) {              // v[1]: x, v[2]: y
      for (int r = 0; r < 2; ++r) {
        if (v[1 + r] == 0.) continue;
        for (int k = 0; k < 3; ++k) { A[r * 3 + k] = -A[r * 3 + k]; Rn[r * 3 + k] = -Rn[r * 3 + k]; }
        t[r] = -t[r];
        const double a = -hi[r], b = -lo[r];
        lo[r] = a;
        hi[r] = b;
      }
    } else if (kind == AU_SHIFT) {             // v[1..4)
      for (int q = 0; q < 3; ++q) { t[q] += v[1 + q]; lo[q] += v[1 + q]; hi[q] += v[1 + q]; }
    }
  }
  for (int q = 0; q < 9; ++q) { aff[q] = A[q]; aff[12 + q] = Rn[q]; }
  for (int q = 0; q < 3; ++q) aff[9 + q] = t[q];
  if (stats && !rotated) {
    for (int q = 0; q < 3; ++q) { stats[q] = lo[q]; stats[3 + q] = hi[q]; }
  }
}

// ---- the flush ---------------------------------------------------------------------------------------------------------------------------
template <bool STATS>
__global__ void __launch_bounds__(AU_THREADS)
aug_apply_kernel(AuApply a, double* __restrict__ partial) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const uint64_t jkey = au_key(a.jseed, 0);
  double m[21];
  if (a.aff) {
#pragma unroll
    for (int q = 0; q < 21; ++q) m[q] = a.aff[q];
  }
  float cl[3] = {0.f, 0.f, 0.f}, ch[3] = {0.f, 0.f, 0.f};
  if (a.color_out && a.stats) {
#pragma unroll
    for (int q = 0; q < 3; ++q) { cl[q] = (float)a.stats[6 + q]; ch[q] = (float)a.stats[9 + q]; }
  }
  for (int k = 0; k < AU_PPT; ++k) {
    const int64_t i = (int64_t)blockIdx.x * AU_TILE + k * AU_THREADS + threadIdx.x;
    if (i >= a.n) continue;
    if (a.coord_out) {
      const float x = a.coord[i * 3], y = a.coord[i * 3 + 1], z = a.coord[i * 3 + 2];
      float o[3] = {x, y, z};
      if (a.aff || a.jitter) {
        double p[3] = {(double)x, (double)y, (double)z};
        if (a.aff) au_affine(m, x, y, z, p[0], p[1], p[2]);
        if (a.jitter) {
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const float zn = a.jnoise ? a.jnoise[i * 3 + q] : au_normal(jkey, (uint64_t)i * 3 + q);
            p[q] += fmin(fmax(a.sigma * (double)zn, -a.jclip), a.jclip);
          }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) o[q] = (float)p[q];
      }
      if (a.pclip) {
#pragma unroll
        for (int q = 0; q < 3; ++q) o[q] = fminf(fmaxf(o[q], (float)a.range[q]), (float)a.range[3 + q]);
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        a.coord_out[i * 3 + q] = o[q];
        if (STATS) { lo[q] = fmin(lo[q], (double)o[q]); hi[q] = fmax(hi[q], (double)o[q]); }
      }
    }
    if (a.normal_out) {
      const float x = a.normal[i * 3], y = a.normal[i * 3 + 1], z = a.normal[i * 3 + 2];
      float o[3] = {x, y, z};
      if (a.aff) {
        const double* r = m + 12;
#pragma unroll
        for (int q = 0; q < 3; ++q)
          o[q] = (float)fma(r[q * 3], (double)x, fma(r[q * 3 + 1], (double)y, r[q * 3 + 2] * (double)z));
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) a.normal_out[i * 3 + q] = o[q];
    }
    if (a.color_out) {
      float c[3] = {a.color[i * 3], a.color[i * 3 + 1], a.color[i * 3 + 2]};
      for (int op = 0; op < a.ncolor; ++op) {
        const int kind = a.ckind[op];
        if (kind == AU_C_AUTOCONTRAST) {          // cpar[0]: the blend factor
          const float* l = cl;
          const float* h = ch;
          if (h[0] > l[0] || h[1] > l[1] || h[2] > l[2]) {
            const float b = a.cpar[op][0];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              const float scale = h[q] > l[q] ? 255.f / (h[q] - l[q]) : 1.f;
              c[q] = (1.f - b) * c[q] + b * ((c[q] - l[q]) * scale);
            }
          }
        } else if (kind == AU_C_TRANSLATION) {    // cpar[0..3): the shift
#pragma unroll
          for (int q = 0; q < 3; ++q) c[q] = fminf(fmaxf(a.cpar[op][q] + c[q], 0.f), 255.f);
        } else if (kind == AU_C_JITTER) {         // cpar[0]: std * 255
          const uint64_t ck = au_key(a.cseed[op], a.cstream[op]);
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const float zn = a.cnoise[op] ? a.cnoise[op][i * 3 + q] : au_normal(ck, (uint64_t)i * 3 + q);
            c[q] = fminf(fmaxf(zn * a.cpar[op][0] + c[q], 0.f), 255.f);
          }
        } else {                                  // AU_C_NORMALIZE
#pragma unroll
          for (int q = 0; q < 3; ++q) c[q] = c[q] / 255.f;
        }
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) a.color_out[i * 3 + q] = c[q];
    }
  }
  if (STATS) au_block_minmax<3>(lo, hi, partial + (int64_t)blockIdx.x * 6);
}

__global__ void __launch_bounds__(AU_THREADS)
aug_noise_kernel(uint64_t key, int64_t count, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * AU_THREADS + threadIdx.x;
  if (e < count) out[e] = au_normal(key, (uint64_t)e);
}

// ---- elastic distortion -------------------------------------------------------------------------------------------------------------------
// 9 M[i][a] of the closed form: the number of k in [0, dim) with |i - k| <= 1 and |k - a| <= 1
__device__ __forceinline__ int au_taps(int i, int a, int dim) {
  const int lo = max(max(i, a) - 1, 0), hi = min(min(i, a) + 1, dim - 1);
  return max(hi - lo + 1, 0);
}

__global__ void __launch_bounds__(AU_THREADS)
aug_elastic_grid_kernel(const float* __restrict__ noise, int dx, int dy, int dz, float* __restrict__ grid) {
  const int64_t o = (int64_t)blockIdx.x * AU_THREADS + threadIdx.x;
  if (o >= (int64_t)dx * dy * dz * 3) return;
  const int ch = (int)(o % 3);
  int64_t r = o / 3;
  const int k = (int)(r % dz);
  r /= dz;
  const int j = (int)(r % dy), i = (int)(r / dy);
  double acc = 0.;          // 125 integer-weighted taps summed in double, one division and one rounding
  for (int a = max(i - 2, 0); a <= min(i + 2, dx - 1); ++a) {
    const int wx = au_taps(i, a, dx);
    for (int b = max(j - 2, 0); b <= min(j + 2, dy - 1); ++b) {
      const int wxy = wx * au_taps(j, b, dy);
      for (int c = max(k - 2, 0); c <= min(k + 2, dz - 1); ++c)
        acc += (double)(wxy * au_taps(k, c, dz)) * (double)noise[(((int64_t)a * dy + b) * dz + c) * 3 + ch];
    }
  }
  grid[o] = (float)(acc / 729.);
}

__global__ void __launch_bounds__(AU_THREADS)
aug_elastic_apply_kernel(const float* __restrict__ coord, int64_t n, const double* __restrict__ aff, const double* __restrict__ stats,
                         const float* __restrict__ grid, int dx, int dy, int dz, double g, double magnitude, float* __restrict__ out,
                         double* __restrict__ partial) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const float mn[3] = {(float)stats[0], (float)stats[1], (float)stats[2]};     // rounding is monotonic: the min of the rounded points
  const int dim[3] = {dx, dy, dz};
  double m[12];
  if (aff) {
#pragma unroll
    for (int q = 0; q < 12; ++q) m[q] = aff[q];
  }
  for (int k = 0; k < AU_PPT; ++k) {
    const int64_t i = (int64_t)blockIdx.x * AU_TILE + k * AU_THREADS + threadIdx.x;
    if (i >= n) continue;
    const float x = coord[i * 3], y = coord[i * 3 + 1], z = coord[i * 3 + 2];
    float p[3] = {x, y, z};
    if (aff) {
      double q[3];
      au_affine(m, x, y, z, q[0], q[1], q[2]);
      p[0] = (float)q[0]; p[1] = (float)q[1]; p[2] = (float)q[2];
    }
    int c[3];
    float f[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      // the grid starts at min - g.  The cell coordinate is formed in double (g = 0.2 is not an fp32 number: (p - min) / g in fp32
      // would carry its rounding times the number of cells); the interpolation itself is fp32
      const double u = ((double)p[q] - (double)mn[q]) / g + 1.;
      int ci = (int)floor(u);
      ci = min(max(ci, 0), dim[q] - 2);                 // an offset that is an exact multiple of g at the upper bound: index dim - 1
      c[q] = ci;
      f[q] = (float)(u - (double)ci);
    }
    const float* base = grid + (((int64_t)c[0] * dy + c[1]) * dz + c[2]) * 3;
    const int64_t sx = (int64_t)dy * dz * 3, sy = (int64_t)dz * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float v000 = base[ch], v001 = base[3 + ch], v010 = base[sy + ch], v011 = base[sy + 3 + ch];
      const float v100 = base[sx + ch], v101 = base[sx + 3 + ch], v110 = base[sx + sy + ch], v111 = base[sx + sy + 3 + ch];
      const float v00 = v000 + f[2] * (v001 - v000), v01 = v010 + f[2] * (v011 - v010);
      const float v10 = v100 + f[2] * (v101 - v100), v11 = v110 + f[2] * (v111 - v110);
      const float v0 = v00 + f[1] * (v01 - v00), v1 = v10 + f[1] * (v11 - v10);
      const float o = (float)fma((double)(v0 + f[0] * (v1 - v0)), magnitude, (double)p[ch]);      // one rounding
      out[i * 3 + ch] = o;
      lo[ch] = fmin(lo[ch], (double)o);
      hi[ch] = fmax(hi[ch], (double)o);
    }
  }
  au_block_minmax<3>(lo, hi, partial + (int64_t)blockIdx.x * 6);
}

// ------------------------------------------------------------------------------------------------
extern "C" int64_t ptc_aug_abi(void) { return PTC_AUG_ABI; }

extern "C" int64_t ptc_aug_partials(int64_t n) { return n > 0 ? ptc_cdiv(n, AU_TILE) : 1; }

extern "C" int ptc_aug_reduce(const float* coord, const float* color, int64_t n, const double* aff, double* partial, double* stats,
                              ptc_stream_t stream) {
  PTC_REQUIRE(n >= 1, PTC_EINVAL, "ptc_aug_reduce: empty point cloud");
  PTC_REQUIRE((coord || color) && partial && stats, PTC_EINVAL, "ptc_aug_reduce: null buffer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = ptc_aug_partials(n);
  hipLaunchKernelGGL(aug_reduce_kernel, dim3((unsigned)rows), dim3(AU_THREADS), 0, s, coord, color, n, aff, partial);
  PTC_CHECK_LAUNCH("aug_reduce_kernel");
  // a part that was not asked for keeps its statistics
  hipLaunchKernelGGL(aug_finish_kernel, dim3(1), dim3(AU_THREADS), 0, s, (const double*)partial, rows, 12, coord ? 0 : 6,
                     coord && color ? 12 : 6, stats);
  PTC_CHECK_LAUNCH("aug_finish_kernel");
  return PTC_OK;
}

extern "C" int ptc_aug_compose(const double* ops, int n_ops, int from_identity, double* aff, double* stats, ptc_stream_t stream) {
  PTC_REQUIRE(n_ops >= 0 && n_ops <= AU_MAX_OPS, PTC_EINVAL, "ptc_aug_compose: %d descriptors (at most %d per call)", n_ops, AU_MAX_OPS);
  PTC_REQUIRE(aff && (ops || n_ops == 0), PTC_EINVAL, "ptc_aug_compose: null buffer");
  AuOps o;
  o.n = n_ops;
  for (int i = 0; i < n_ops; ++i) {
    const int kind = (int)ops[i * 8];
    PTC_REQUIRE(kind >= AU_CENTER_SHIFT && kind <= AU_SHIFT, PTC_EINVAL, "ptc_aug_compose: bad descriptor kind %d", kind);
    const bool needs_box = kind == AU_CENTER_SHIFT || (kind == AU_ROTATE && ops[i * 8 + 4] == 0.);
    PTC_REQUIRE(!needs_box || stats, PTC_EINVAL, "ptc_aug_compose: descriptor %d needs the bounding box (stats)", i);
    for (int q = 0; q < 8; ++q) o.v[i][q] = ops[i * 8 + q];
  }
  hipLaunchKernelGGL(aug_compose_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, o, from_identity, aff, stats);
  PTC_CHECK_LAUNCH("aug_compose_kernel");
  return PTC_OK;
}

extern "C" int ptc_aug_apply(const float* coord, const float* normal, const float* color, int64_t n, const double* aff, const double* stats,
                             int jitter, double sigma, double clip, const float* jitter_noise, uint64_t jitter_seed,
                             const double* clip_range, const double* color_ops, const float* const* color_noise, int n_color_ops,
                             float* coord_out, float* normal_out, float* color_out, double* partial, double* stats_out,
                             ptc_stream_t stream) {
  PTC_REQUIRE(n >= 1, PTC_EINVAL, "ptc_aug_apply: empty point cloud");
  PTC_REQUIRE(n_color_ops >= 0 && n_color_ops <= AU_MAX_COLOR, PTC_EINVAL, "ptc_aug_apply: %d colour ops (at most %d per call)",
              n_color_ops, AU_MAX_COLOR);
  PTC_REQUIRE((!coord_out || coord) && (!normal_out || normal) && (!color_out || color), PTC_EINVAL, "ptc_aug_apply: an output without its input");
  PTC_REQUIRE(coord_out || normal_out || color_out, PTC_EINVAL, "ptc_aug_apply: nothing to write");
  PTC_REQUIRE((!jitter && !clip_range && !partial) || coord_out, PTC_EINVAL, "ptc_aug_apply: jitter / clip / statistics need coordinates");
  PTC_REQUIRE(!jitter || clip > 0., PTC_EINVAL, "ptc_aug_apply: RandomJitter's clip must be positive");
  PTC_REQUIRE(!partial == !stats_out, PTC_EINVAL, "ptc_aug_apply: partial and stats_out go together");
  PTC_REQUIRE(n_color_ops == 0 || (color_out && color_ops), PTC_EINVAL, "ptc_aug_apply: colour ops without a colour tensor");
  AuApply a;
  a.coord = coord; a.normal = normal; a.color = color;
  a.coord_out = coord_out; a.normal_out = normal_out; a.color_out = color_out;
  a.aff = aff; a.stats = stats; a.n = n;
  a.jitter = jitter != 0; a.pclip = clip_range != nullptr; a.ncolor = n_color_ops;
  a.sigma = sigma; a.jclip = clip; a.jnoise = jitter_noise; a.jseed = jitter_seed;
  for (int q = 0; q < 6; ++q) a.range[q] = clip_range ? clip_range[q] : 0.;
  for (int i = 0; i < AU_MAX_COLOR; ++i) {
    a.ckind[i] = AU_C_NORMALIZE; a.cstream[i] = 0; a.cnoise[i] = nullptr; a.cseed[i] = 0;
    a.cpar[i][0] = a.cpar[i][1] = a.cpar[i][2] = 0.f;
  }
  for (int i = 0; i < n_color_ops; ++i) {      // rows of 6: kind, three parameters, seed (< 2^53), stream
    const double* r = color_ops + i * 6;
    const int kind = (int)r[0];
    PTC_REQUIRE(kind >= AU_C_AUTOCONTRAST && kind <= AU_C_NORMALIZE, PTC_EINVAL, "ptc_aug_apply: bad colour op kind %d", kind);
    PTC_REQUIRE(kind != AU_C_AUTOCONTRAST || stats, PTC_EINVAL, "ptc_aug_apply: ChromaticAutoContrast needs the colour statistics");
    a.ckind[i] = kind;
    for (int q = 0; q < 3; ++q) a.cpar[i][q] = (float)r[1 + q];
    a.cseed[i] = (uint64_t)r[4];
    a.cstream[i] = (int)r[5];
    a.cnoise[i] = color_noise ? color_noise[i] : nullptr;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = ptc_aug_partials(n);
  if (partial) {
    hipLaunchKernelGGL(aug_apply_kernel<true>, dim3((unsigned)rows), dim3(AU_THREADS), 0, s, a, partial);
    PTC_CHECK_LAUNCH("aug_apply_kernel");
    hipLaunchKernelGGL(aug_finish_kernel, dim3(1), dim3(AU_THREADS), 0, s, (const double*)partial, rows, 6, 0, 6, stats_out);
    PTC_CHECK_LAUNCH("aug_finish_kernel");
  } else {
    hipLaunchKernelGGL(aug_apply_kernel<false>, dim3((unsigned)rows), dim3(AU_THREADS), 0, s, a, (double*)nullptr);
    PTC_CHECK_LAUNCH("aug_apply_kernel");
  }
  return PTC_OK;
}

extern "C" int ptc_aug_noise(uint64_t seed, int stream_id, int64_t count, float* out, ptc_stream_t stream) {
  PTC_REQUIRE(count >= 0 && stream_id >= 0, PTC_EINVAL, "ptc_aug_noise: bad sizes");
  if (count == 0) return PTC_OK;
  PTC_REQUIRE(out, PTC_EINVAL, "ptc_aug_noise: null buffer");
  hipLaunchKernelGGL(aug_noise_kernel, dim3((unsigned)ptc_cdiv(count, AU_THREADS)), dim3(AU_THREADS), 0, (hipStream_t)stream,
                     au_key(seed, stream_id), count, out);
  PTC_CHECK_LAUNCH("aug_noise_kernel");
  return PTC_OK;
}

extern "C" int ptc_aug_elastic_grid(float* noise, int generate, uint64_t seed, int stream_id, int dx, int dy, int dz, float* grid,
                                    ptc_stream_t stream) {
  PTC_REQUIRE(dx >= 2 && dy >= 2 && dz >= 2 && (int64_t)dx * dy * dz <= ((int64_t)1 << 28), PTC_EINVAL,
              "ptc_aug_elastic_grid: grid %d x %d x %d", dx, dy, dz);
  PTC_REQUIRE(noise && grid && noise != grid, PTC_EINVAL, "ptc_aug_elastic_grid: null or aliased buffer");
  const int64_t count = (int64_t)dx * dy * dz * 3;
  if (generate) {
    if (int rc = ptc_aug_noise(seed, stream_id, count, noise, stream)) return rc;
  }
  hipLaunchKernelGGL(aug_elastic_grid_kernel, dim3((unsigned)ptc_cdiv(count, AU_THREADS)), dim3(AU_THREADS), 0, (hipStream_t)stream,
                     (const float*)noise, dx, dy, dz, grid);
  PTC_CHECK_LAUNCH("aug_elastic_grid_kernel");
  return PTC_OK;
}

extern "C" int ptc_aug_elastic_apply(const float* coord, int64_t n, const double* aff, const double* stats, const float* grid, int dx,
                                     int dy, int dz, double granularity, double magnitude, float* coord_out, double* partial,
                                     double* stats_out, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 1, PTC_EINVAL, "ptc_aug_elastic_apply: empty point cloud");
  PTC_REQUIRE(dx >= 2 && dy >= 2 && dz >= 2 && granularity > 0., PTC_EINVAL, "ptc_aug_elastic_apply: grid %d x %d x %d, granularity %g",
              dx, dy, dz, granularity);
  PTC_REQUIRE(coord && stats && grid && coord_out && partial && stats_out, PTC_EINVAL, "ptc_aug_elastic_apply: null buffer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = ptc_aug_partials(n);
  hipLaunchKernelGGL(aug_elastic_apply_kernel, dim3((unsigned)rows), dim3(AU_THREADS), 0, s, coord, n, aff, stats, grid, dx, dy, dz,
                     granularity, magnitude, coord_out, partial);
  PTC_CHECK_LAUNCH("aug_elastic_apply_kernel");
  hipLaunchKernelGGL(aug_finish_kernel, dim3(1), dim3(AU_THREADS), 0, s, (const double*)partial, rows, 6, 0, 6, stats_out);
  PTC_CHECK_LAUNCH("aug_finish_kernel");
  return PTC_OK;
}
