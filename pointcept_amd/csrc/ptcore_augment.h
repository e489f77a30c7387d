/*
 * ptcore_augment.h -- the device-side point augmentation section of libptcore.so's C-ABI (csrc/augment.hip).
 *
 * Same boundary contract as include/ptcore.h (extern "C", caller-owned buffers, statuses, streams; its ERRORS rule holds here:
 * an `int` entry point whose last parameter is the ptc_stream_t returns a status, everything else takes scalars and returns a
 * value).  It is a header of its own because include/ptcore.h is the pinned surface of the backbone engine; the ctypes binding
 * (pointcept_amd/_lib.py) derives these signatures from this file in the same way, and checks PTC_AUG_ABI against the library.
 */
#ifndef PTCORE_AUGMENT_H
#define PTCORE_AUGMENT_H

#include "../../include/ptcore.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever a declaration below changes; ptc_aug_abi() returns the value the library was compiled with */
#define PTC_AUG_ABI 1
int64_t ptc_aug_abi(void);

#define PTC_AUG_MAX_OPS 16            /* limits and kinds, their one definition: affine descriptors per ptc_aug_compose call */
#define PTC_AUG_MAX_COLOR_OPS 8       /* colour ops per ptc_aug_apply call */
enum ptc_aug_kind { PTC_AUG_CENTER_SHIFT = 0, PTC_AUG_ROTATE = 1, PTC_AUG_SCALE = 2, PTC_AUG_FLIP = 3, PTC_AUG_SHIFT = 4 };
enum ptc_aug_color_kind { PTC_AUG_C_AUTOCONTRAST = 0, PTC_AUG_C_TRANSLATION = 1, PTC_AUG_C_JITTER = 2, PTC_AUG_C_NORMALIZE = 3 };

/* ------------------------------------------------------------------------------------------
 * Device-side point augmentation (csrc/augment.hip; pointcept/datasets/transform.py:143-451, :779-836).
 * State of one scene, on the device in double: aff [21] = A [3x3] row-major, t [3], Rn [3x3] (coord' = A p + t, normal' = Rn n) and
 *   stats [12] = min xyz, max xyz of the cloud under the pending affine, min rgb, max rgb of the colours.  coord / normal / color are
 *   [n,3] fp32, n >= 1.  aff == NULL means the identity.  partial: ptc_aug_partials(n) rows of 12 (ptc_aug_reduce) or 6 doubles.
 *   Nothing here synchronises or reads device memory on the host; min / max are exact, no atomics: bit-reproducible.
 * ptc_aug_reduce: stats[0..6) = box of A p + t when coord != NULL, stats[6..12) = channel min / max when color != NULL; the other
 *   half of stats keeps its values.
 * ptc_aug_compose: ops = HOST [n_ops, 8] doubles (n_ops <= PTC_AUG_MAX_OPS), each row kind (enum ptc_aug_kind) then arguments:
 *     0 CenterShift(apply_z)                      shift by -((xmin+xmax)/2, (ymin+ymax)/2, apply_z ? zmin : 0)             needs stats
 *     1 Rotate(axis 0|1|2, cos, sin, given, cx, cy, cz)  about the given centre, or (given == 0) the box centre            needs stats
 *     2 Scale(sx, sy, sz)     3 Flip(x, y)     4 Shift(dx, dy, dz)
 *   from_identity != 0: aff is written without being read.  The box in stats is carried through kinds 0, 2, 3, 4 and written back; after
 *   a Rotate stats[0..6) is left as it was and no longer describes the cloud (reduce again before the next op that needs the box).
 * ptc_aug_apply: the flush; every part is optional (an output pointer NULL: part absent; in place is allowed).
 *     coord_out = A p + t, evaluated in double, + clip(sigma z, -clip, clip) when jitter != 0 (z = jitter_noise [n,3], or NULL: the
 *       generator with (jitter_seed, stream 0)), rounded once, then clamped to clip_range (HOST [6] = min xyz, max xyz; NULL: none).
 *     normal_out = Rn n.
 *     color_out = the n_color_ops <= PTC_AUG_MAX_COLOR_OPS ops of color_ops (HOST [n,6] doubles: kind (enum ptc_aug_color_kind), p0, p1, p2, seed < 2^53, stream) in order, fp32:
 *       0 AutoContrast(blend): lo / hi = stats[6..12); scale 255 / (hi - lo), 1 on a channel with hi == lo; untouched when no channel
 *         differs; (1 - blend) c + blend (c - lo) scale       1 Translation(r, g, b): clip(t + c, 0, 255)
 *       2 Jitter(std * 255): clip(z p0 + c, 0, 255), z = color_noise[i] [n,3] (HOST array of n_color_ops device pointers, or NULL) or
 *         the generator with (seed, stream)                     3 Normalize: c / 255
 *     partial / stats_out (both or neither): the box of coord_out -> stats_out[0..6).
 * ptc_aug_noise: out[e] = z(seed, stream_id, e), e < count: the counter-based standard normal every consumer above evaluates in place
 *   (a pure function of its three arguments).
 * ptc_aug_elastic_grid: grid [dx,dy,dz,3] fp32 = the noise [dx,dy,dz,3] after the reference's two rounds of width-3 box filters along
 *   x, y, z with zero padding, as one closed-form stencil (125 taps, summed in double).  generate != 0: noise is first filled by the
 *   generator with (seed, stream_id); otherwise it is the caller's standard-normal tensor.  dx, dy, dz >= 2.
 * ptc_aug_elastic_apply: p = A p0 + t rounded to fp32, u = (p - min) / g + 1 in double with min = stats[0..3) rounded to fp32,
 *   cell = floor(u) clamped to [0, dim - 2], trilinear interpolation of the grid in fp32 at u - cell, coord_out = p + interp *
 *   magnitude rounded once; stats_out[0..6) = the box of coord_out.
 * ------------------------------------------------------------------------------------------ */
int64_t ptc_aug_partials(int64_t n);
int ptc_aug_reduce(const float* coord, const float* color, int64_t n, const double* aff, double* partial, double* stats,
                   ptc_stream_t stream);
int ptc_aug_compose(const double* ops, int n_ops, int from_identity, double* aff, double* stats, ptc_stream_t stream);
int ptc_aug_apply(const float* coord, const float* normal, const float* color, int64_t n, const double* aff, const double* stats,
                  int jitter, double sigma, double clip, const float* jitter_noise, uint64_t jitter_seed, const double* clip_range,
                  const double* color_ops, const float* const* color_noise, int n_color_ops, float* coord_out, float* normal_out,
                  float* color_out, double* partial, double* stats_out, ptc_stream_t stream);
int ptc_aug_noise(uint64_t seed, int stream_id, int64_t count, float* out, ptc_stream_t stream);
int ptc_aug_elastic_grid(float* noise, int generate, uint64_t seed, int stream_id, int dx, int dy, int dz, float* grid,
                         ptc_stream_t stream);
int ptc_aug_elastic_apply(const float* coord, int64_t n, const double* aff, const double* stats, const float* grid, int dx, int dy,
                          int dz, double granularity, double magnitude, float* coord_out, double* partial, double* stats_out,
                          ptc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PTCORE_AUGMENT_H */
