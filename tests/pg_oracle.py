"""TEST INFRASTRUCTURE.  A line-by-line Python restatement of libs/pointgroup_ops (the reference's CUDA extension, which needs nvcc and
Google sparsehash and cannot be built here): ballquery_batch_p_cuda_ (bfs_cluster_kernel.cu:16-61) and get_clusters / find_cc /
fill_cluster_idxs_ (bfs_cluster.cpp:53-123), in numpy float32 with the reference's unfused d2 expression.  Also a stand-in
`pointgroup_ops` module (ballquery_batch_p, bfs_cluster on CPU tensors) for running the reference's model file on the CPU."""
from collections import deque
import types

import numpy as np
import torch

MAX_NBR = 1000


def ballquery_batch_p(xyz, batch_idxs, batch_offsets, radius):
    """-> (idx int32 [nActive], start_len int32 [n, 2]); starts as the exclusive scan of the lengths (the reference's atomicAdd
    cursor orders them arbitrarily; the lists themselves are the reference's)."""
    xyz = np.asarray(xyz, dtype=np.float32)
    batch_idxs = np.asarray(batch_idxs).astype(np.int64)
    off = np.asarray(batch_offsets).astype(np.int64)
    n = xyz.shape[0]
    r2 = np.float32(radius) * np.float32(radius)
    lists = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            b = batch_idxs[i]
            s, e = off[b], off[b + 1]
            o = xyz[i]
            seg = xyz[s:e]
            dx = o[0] - seg[:, 0]
            dy = o[1] - seg[:, 1]
            dz = o[2] - seg[:, 2]
            d2 = (dx * dx + dy * dy) + dz * dz        # float32 throughout, the kernel's left-to-right order
            hit = np.nonzero(d2 < r2)[0][:MAX_NBR] + s
            lists.append(hit.astype(np.int32))
    lens = np.asarray([len(h) for h in lists], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if n else np.zeros(0, np.int64)
    start_len = np.stack([starts, lens], 1).astype(np.int32) if n else np.zeros((0, 2), np.int32)
    idx = np.concatenate(lists).astype(np.int32) if n and lens.sum() else np.zeros(0, np.int32)
    return idx, start_len


def bfs_cluster(label, idx, start_len, threshold):
    """-> (cluster_idxs int32 [sumNPoint, 2] with members in BFS order, cluster_offsets int32 [nCluster + 1])"""
    label = np.asarray(label)
    idx = np.asarray(idx)
    start_len = np.asarray(start_len)
    n = start_len.shape[0]
    visited = np.zeros(n, dtype=bool)
    clusters = []
    for i in range(n):
        if visited[i]:
            continue
        cc = [i]
        visited[i] = True
        q = deque([i])
        while q:
            cur = q.popleft()
            s, ln = int(start_len[cur, 0]), int(start_len[cur, 1])
            lc = label[cur]
            for j in idx[s:s + ln]:
                j = int(j)
                if label[j] != lc or visited[j]:
                    continue
                cc.append(j)
                visited[j] = True
                q.append(j)
        if len(cc) >= threshold:
            clusters.append(cc)
    offsets = np.zeros(len(clusters) + 1, dtype=np.int32)
    rows = []
    for k, cc in enumerate(clusters):
        offsets[k + 1] = offsets[k] + len(cc)
        rows += [(k, p) for p in cc]
    cidx = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    return cidx, offsets


def canonical(cidx, coff):
    """(offsets, seeds, sorted member arrays) -- what the engine must reproduce exactly"""
    cidx = np.asarray(cidx).reshape(-1, 2)
    coff = np.asarray(coff)
    seeds = [int(cidx[coff[k], 1]) for k in range(len(coff) - 1)]
    members = [np.sort(cidx[coff[k]:coff[k + 1], 1]) for k in range(len(coff) - 1)]
    assert all(int((cidx[coff[k]:coff[k + 1], 0] != k).sum()) == 0 for k in range(len(coff) - 1))
    return coff.astype(np.int64), seeds, members


def assert_same_clusters(a, b):
    oa, sa, ma = canonical(*a)
    ob, sb, mb = canonical(*b)
    assert np.array_equal(oa, ob), "cluster offsets differ"
    assert sa == sb, "cluster seeds differ"
    for x, y in zip(ma, mb):
        assert np.array_equal(x, y), "cluster members differ"


def stand_in_module():
    """`pointgroup_ops` for the reference's model file on CPU tensors (point_group_v1m1_base.py:13-16 imports these two names)"""
    m = types.ModuleType("pointgroup_ops")

    def bq(coords, batch_idxs, batch_offsets, radius, mean_active):
        idx, sl = ballquery_batch_p(coords.detach().float().cpu().numpy(), batch_idxs.cpu().numpy(), batch_offsets.cpu().numpy(), radius)
        return torch.from_numpy(idx), torch.from_numpy(sl)

    def bfs(label, idx, start_len, threshold):
        ci, co = bfs_cluster(label.numpy(), idx.numpy(), start_len.numpy(), threshold)
        return torch.from_numpy(ci), torch.from_numpy(co)

    m.ballquery_batch_p, m.bfs_cluster = bq, bfs
    return m
