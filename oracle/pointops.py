"""TEST INFRASTRUCTURE (oracle).  numpy restatements of the pointops query / sampling kernels that exist only as CUDA in the
reference (libs/pointops/src/knn_query/knn_query_cuda_kernel.cu:60-108, src/sampling/sampling_cuda_kernel.cu:15-122, the two ball
queries), and of the python wrapper built on the k-NN (functions/interpolation.py, float64) --
"parity unpinned": they cannot be executed here; semantics follow the kernels' loops, with the tie order the reference
leaves implementation-defined fixed to "lower index first".  fp32 arithmetic, ((dx*dx + dy*dy) + dz*dz), like the kernels."""
from __future__ import annotations

import numpy as np


def _d2(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    d = (a.astype(np.float32) - b.astype(np.float32))
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def knn_query(nsample, xyz, offset, new_xyz, new_offset):
    m = new_xyz.shape[0]
    idx = np.full((m, nsample), -1, dtype=np.int32)
    d2 = np.full((m, nsample), np.float32(1e10), dtype=np.float32)
    s0 = q0 = 0
    for s1, q1 in zip(offset, new_offset):
        pts = xyz[s0:s1]
        for q in range(q0, q1):
            d = _d2(pts, new_xyz[q][None, :])
            order = np.lexsort((np.arange(len(d)), d))[:nsample]
            idx[q, : len(order)] = order + s0
            d2[q, : len(order)] = d[order]
        s0, q0 = s1, q1
    return idx, np.sqrt(d2)


def farthest_point_sampling(xyz, offset, new_offset):
    out = np.zeros(int(new_offset[-1]), dtype=np.int32)
    s0 = q0 = 0
    for s1, q1 in zip(offset, new_offset):
        if q1 > q0 and s1 > s0:
            tmp = np.full(s1 - s0, np.float32(1e10), dtype=np.float32)
            old = s0
            out[q0] = s0
            for j in range(q0 + 1, q1):
                tmp = np.minimum(_d2(xyz[s0:s1], xyz[old][None, :]), tmp)
                old = s0 + int(np.argmax(tmp))          # first maximum = lowest index
                out[j] = old
        s0, q0 = s1, q1
    return out


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3, grad_out=None):
    """libs/pointops/functions/interpolation.py:8-24 in float64 over this file's knn_query (fp32 distances, as the wrapper
    receives them): recip = 1 / (dist + 1e-8), weight = recip / recip.sum(1), out = sum_i weight_i feat[idx_i].  A -1 slot
    (scene with fewer than k points: dist 1e5) keeps its ~1e-5 share of the normaliser and contributes zero -- the port's
    grouping convention; the reference indexes feat[-1] there.  -> out [m, c], or (out, d_feat [n, c]) for a given
    grad_out [m, c]: the transposed weighted scatter (interpolation_backward_cuda)."""
    idx, dist = knn_query(k, xyz, offset, new_xyz, new_offset)
    recip = 1.0 / (dist.astype(np.float64) + 1e-8)
    weight = recip / recip.sum(1, keepdims=True)
    feat = np.asarray(feat, dtype=np.float64)
    live = idx >= 0
    safe = np.where(live, idx, 0)
    w = np.where(live, weight, 0.0)
    out = (w[:, :, None] * feat[safe]).sum(1)
    if grad_out is None:
        return out
    d_feat = np.zeros_like(feat)
    np.add.at(d_feat, safe.reshape(-1), (w[:, :, None] * np.asarray(grad_out, dtype=np.float64)[:, None, :]).reshape(-1, feat.shape[1]))
    return out, d_feat


def ball_query(nsample, max_radius, min_radius, xyz, offset, new_xyz, new_offset, order=None):
    """libs/pointops/src/ball_query/ball_query_cuda_kernel.cu:59-123 (order=None) and
    src/random_ball_query/random_ball_query_cuda_kernel.cu:58-108 (order = permutation): -> (idx, dist) with dist = sqrt(dist2)
    as the python wrappers return (functions/query.py:75,113).  Ties: lower index first.  The sub-sampled branch returns the
    candidate's distance (the CUDA kernel writes the candidate index into dist2 there, :120)."""
    m = new_xyz.shape[0]
    idx = np.full((m, nsample), -1, dtype=np.int32)
    d2o = np.full((m, nsample), np.float32(1e10), dtype=np.float32)
    mn, mx = np.float32(min_radius) * np.float32(min_radius), np.float32(max_radius) * np.float32(max_radius)
    s0 = q0 = 0
    for s1, q1 in zip(offset, new_offset):
        cand_ids = np.arange(s0, s1) if order is None else np.asarray(order[s0:s1])
        pts = xyz[cand_ids]
        for q in range(q0, q1):
            d = _d2(pts, new_xyz[q][None, :])
            inr = (d <= np.float32(1e-5)) | ((d >= mn) & (d < mx))
            ci, cd = cand_ids[inr], d[inr]
            if order is None:
                ci, cd = ci[:2048], cd[:2048]                      # the kernel's candidate array bound
                o = np.lexsort((ci, cd))
                ci, cd = ci[o], cd[o]
                if len(ci) > nsample:
                    sep = np.float32(len(ci)) / np.float32(nsample)
                    pick = (sep * np.arange(nsample, dtype=np.float32)).astype(np.int32)
                    ci, cd = ci[pick], cd[pick]
            else:
                ci, cd = ci[:nsample], cd[:nsample]
            idx[q, :len(ci)] = ci
            d2o[q, :len(ci)] = cd
        s0, q0 = s1, q1
    return idx, np.sqrt(d2o)
