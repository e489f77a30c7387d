"""Mirror of the two torch_geometric names the reference's OA-CNNs and PTv2 files import
(pointcept/models/oacnns/oacnns_v1m1_base.py:8-9, point_transformer_v2m2_base.py:15):
    torch_geometric.nn.pool.voxel_grid(pos, size, batch=None, start=None, end=None) -> linearised cell ids [N] int64
    torch_geometric.utils.scatter(src, index, dim=0, dim_size=None, reduce="sum" | "mean")
Installed only on request: pointcept_amd.compat.install(geometric=True).

voxel_grid is torch_cluster's grid_cluster on [pos | batch] written as the same fp32 (input dtype) expression: cell =
trunc((pos - start) / size), start = the GLOBAL minimum over the batch, ids linearised with x fastest and the batch index slowest.
scatter sorts the index once (ptc_sort_keys) and reduces with the CSR kernel of rows.hip (sum / mean): no float atomics, so
forward and gradient are bit-reproducible; any other reduce raises PtcoreError.
"""
from __future__ import annotations

import types

import torch

from . import functional as PF
from . import ops
from ._lib import PtcoreError


def voxel_grid(pos, size, batch=None, start=None, end=None):
    pos = pos.unsqueeze(-1) if pos.dim() == 1 else pos
    dim = pos.shape[1]
    if batch is None:
        batch = pos.new_zeros(pos.shape[0], dtype=torch.long)
    p = torch.cat([pos, batch.view(-1, 1).to(pos.dtype)], dim=-1)
    sz = torch.tensor((list(size) if isinstance(size, (list, tuple)) else [float(size)] * dim) + [1.0], dtype=pos.dtype, device=pos.device)
    if start is None:
        st = p.min(0).values
    elif isinstance(start, (list, tuple, torch.Tensor)):
        st = torch.cat([torch.as_tensor(start, dtype=pos.dtype, device=pos.device).reshape(-1), pos.new_zeros(1)])
    else:
        st = torch.tensor([float(start)] * dim + [0.0], dtype=pos.dtype, device=pos.device)
    en = p.max(0).values if end is None else torch.cat(
        [torch.as_tensor(end, dtype=pos.dtype, device=pos.device).reshape(-1), batch.max().to(pos.dtype).reshape(1)])
    num = torch.div(en - st, sz).to(torch.long) + 1
    stride = torch.cat([torch.ones(1, dtype=torch.long, device=pos.device), num.cumprod(0)])[: dim + 1]
    return (torch.div(p - st.unsqueeze(0), sz.unsqueeze(0)).to(torch.long) * stride.unsqueeze(0)).sum(1)


def scatter(src, index, dim=0, dim_size=None, reduce="sum"):
    if reduce not in ("sum", "mean", "add"):
        raise PtcoreError(f"torch_geometric_api.scatter: reduce={reduce!r} is not implemented (sum | mean)")
    if dim not in (0, -src.dim()) or index.dim() != 1 or index.numel() != src.shape[0]:
        raise PtcoreError("torch_geometric_api.scatter: only dim=0 with a 1-D index over the rows is implemented")
    idx = index.to(torch.int64).contiguous()
    n_seg = (int(idx.max()) + 1 if idx.numel() else 0) if dim_size is None else int(dim_size)
    order, _ = ops.sort_keys(idx, 0, max(1, n_seg.bit_length()), want_inverse=False)
    counts = torch.bincount(idx, minlength=n_seg)[:n_seg]
    indptr = torch.zeros(n_seg + 1, dtype=torch.int64, device=src.device)
    torch.cumsum(counts, 0, out=indptr[1:])
    flat = src.reshape(src.shape[0], -1)
    out = PF.segment_csr(flat, indptr, "mean" if reduce == "mean" else "sum", perm=order)
    return out.reshape((n_seg,) + tuple(src.shape[1:]))


nn = types.ModuleType(__name__ + ".nn")
nn.pool = types.ModuleType(__name__ + ".nn.pool")
nn.pool.voxel_grid = voxel_grid
utils = types.ModuleType(__name__ + ".utils")
utils.scatter = scatter
