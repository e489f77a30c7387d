"""Raw (non-differentiable) Python wrappers over the C-ABI of libptcore.so.

Every function takes CUDA tensors, allocates outputs / workspaces as torch tensors, and enqueues
the kernels on torch's current stream.  CPU tensors raise PtcoreError -- there is no fallback.
Differentiable versions live in pointcept_amd/functional.py.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import PtcoreError, check, dtype_code, lib, ptr, require_cuda, stream_ptr  # noqa: F401  (check: for callers of lib(checked=False))

_DT = _lib.DTYPE_CODES      # torch dtype -> ptc_dtype tag
# Limits and code sets are READ from the C-ABI headers (_lib parsed them: no library load); shape rules are ASKED of the library (_ask).
_K, _KA = _lib.HEADER.constants, _lib.AUGMENT_HEADER.constants
ATTN_HEAD_DIM = _K["PTC_ATTN_HEAD_DIM"]      # the base attention kernels, their dropout form and the RPE form (other head dims: attention_hd.h)
EDGE_ROWS_GROUP, EDGE_ROWS_SUB, EDGE_ROWS_REL = (_K["PTC_EDGE_ROWS_" + k] for k in ("GROUP", "SUB", "REL"))     # `mode` of the edge_* ops
EDGE_REDUCE_INTERP, EDGE_REDUCE_AGG, EDGE_REDUCE_POS = (_K["PTC_EDGE_REDUCE_" + k] for k in ("INTERP", "AGG", "POS"))
EDGE_SCATTER_GROUP, EDGE_SCATTER_SUB, EDGE_SCATTER_INTERP, EDGE_SCATTER_AGG = (_K["PTC_EDGE_SCATTER_" + k] for k in ("GROUP", "SUB", "INTERP", "AGG"))
_asked: dict = {}           # (entry point, *scalars) -> its answer


def _ask(name: str, *args):      # a scalar-only predicate / query of the library, asked once per argument tuple
    key = (name,) + args
    r = _asked.get(key)
    if r is None:
        r = _asked[key] = getattr(lib(), name)(*args)
    return r


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------------
# serialization
# ------------------------------------------------------------------------------------------------
def serialize_encode(grid_coord: torch.Tensor, batch: Optional[torch.Tensor], depth: int,
                     orders: Sequence[str]) -> torch.Tensor:
    """serialization.encode for all `orders` at once -> code [k,N] int64
    (pointcept/models/utils/serialization/default.py:8-24)."""
    require_cuda(grid_coord, batch)
    if grid_coord.dtype not in (torch.int64, torch.int32):
        raise PtcoreError(f"grid_coord must be int32/int64, got {grid_coord.dtype}")
    gc = grid_coord.contiguous()
    n = gc.shape[0]
    b = None if batch is None else batch.to(torch.int64).contiguous()
    k = len(orders)
    oc = (ctypes.c_int * k)(*[_lib.ORDER_CODES[o] for o in orders])
    out = torch.empty((k, n), dtype=torch.int64, device=gc.device)
    lib().ptc_serialize_encode(ptr(gc), 1 if gc.dtype == torch.int64 else 0, ptr(b), n, int(depth),
                               ctypes.cast(oc, ctypes.c_void_p), k, ptr(out), stream_ptr())
    return out


def sort_keys(keys: torch.Tensor, begin_bit: int, end_bit: int, want_inverse: bool = True):
    """Stable argsort of every row of keys [k,N] int64 over bits [begin_bit,end_bit) ->
    (order [k,N] int64, inverse [k,N] int64 | None)   (structure.py:93-100)."""
    require_cuda(keys)
    if keys.dtype != torch.int64:
        raise PtcoreError("keys must be int64")
    squeeze = keys.dim() == 1
    k2 = keys.reshape(1, -1) if squeeze else keys
    k2 = k2.contiguous()
    k, n = k2.shape
    order = torch.empty_like(k2)
    inverse = torch.empty_like(k2) if want_inverse else None
    nbytes = lib().ptc_sort_keys_workspace_bytes(n, k)
    ws = _ws(nbytes, k2.device)
    lib().ptc_sort_keys(ptr(k2), n, k, int(begin_bit), int(end_bit), ptr(order), ptr(inverse), ptr(ws), nbytes,
                        stream_ptr())
    if squeeze:
        return order[0], (inverse[0] if want_inverse else None)
    return order, inverse


def exclusive_scan_i32(x: torch.Tensor) -> torch.Tensor:
    require_cuda(x)
    x = x.to(torch.int32).contiguous()
    n = x.numel()
    out = torch.empty(n, dtype=torch.int64, device=x.device)
    nbytes = lib().ptc_exclusive_scan_workspace_bytes(n)
    ws = _ws(nbytes, x.device)
    lib().ptc_exclusive_scan_i32(ptr(x), n, ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------
# patch padding maps
# ------------------------------------------------------------------------------------------------
def pad_sizes(offset_host: Sequence[int], patch: int):
    """(n, n_pad, n_seq) from a host copy of `offset` (ptv3m1:123-138,156-164)."""
    prev, n_pad, n_seq = 0, 0, 0
    for o in offset_host:
        ni = int(o) - prev
        prev = int(o)
        p = ((ni + patch - 1) // patch) * patch if ni > patch else ni
        n_pad += p
        n_seq += (p + patch - 1) // patch
    return prev, n_pad, n_seq


def patch_pad_maps(offset: torch.Tensor, offset_host: Sequence[int], patch: int):
    """SerializedAttention.get_padding_and_inverse (ptv3m1:114-170) in one launch.
    Returns pad [N'] i64, unpad [N] i64, cu_seqlens [n_seq+1] i32, dup [N] i64."""
    require_cuda(offset)
    off = offset.to(torch.int64).contiguous()
    n, n_pad, n_seq = pad_sizes(offset_host, patch)
    dev = off.device
    pad = torch.empty(n_pad, dtype=torch.int64, device=dev)
    unpad = torch.empty(n, dtype=torch.int64, device=dev)
    cu = torch.empty(n_seq + 1, dtype=torch.int32, device=dev)
    dup = torch.empty(n, dtype=torch.int64, device=dev)
    lib().ptc_patch_pad_maps(ptr(off), off.numel(), int(patch), n, n_pad, n_seq, ptr(pad), ptr(unpad), ptr(cu),
                             ptr(dup), stream_ptr())
    return pad, unpad, cu, dup


def attn_tables(order: torch.Tensor, inverse: torch.Tensor, pad: torch.Tensor, unpad: torch.Tensor, dup: torch.Tensor):
    """int32 gather tables of one serialization order (ptv3m1:184-188,216 and their backward) in one launch:
    (t_qkv_fwd [1,N'], t_qkv_bwd [2,N], t_proj_fwd [1,N], t_proj_bwd [1,N'])."""
    require_cuda(order, inverse, pad, unpad, dup)
    n, n_pad = order.numel(), pad.numel()
    dev = order.device
    t1 = torch.empty((1, n_pad), dtype=torch.int32, device=dev)
    t2 = torch.empty((2, n), dtype=torch.int32, device=dev)
    t3 = torch.empty((1, n), dtype=torch.int32, device=dev)
    t4 = torch.empty((1, n_pad), dtype=torch.int32, device=dev)
    lib().ptc_attn_tables(ptr(order.contiguous()), ptr(inverse.contiguous()), ptr(pad), ptr(unpad), ptr(dup), n, n_pad,
                          ptr(t1), ptr(t2), ptr(t3), ptr(t4), stream_ptr())
    return t1, t2, t3, t4


# ------------------------------------------------------------------------------------------------
# pooling maps
# ------------------------------------------------------------------------------------------------
def pool_level_counts(code0: torch.Tensor, order0: torch.Tensor, batch_shift: int, n_batch: int, shifts: Sequence[int]):
    """counts [len(shifts), n_batch] int64 (device): distinct values of code0 >> shifts[l] per scene -- the point counts
    of every pooled level (ptv3m1:384-390), one launch, no sync (the caller fetches them with its own single copy)."""
    require_cuda(code0, order0)
    import ctypes

    counts = torch.empty((len(shifts), n_batch), dtype=torch.int64, device=code0.device)
    arr = (ctypes.c_int * len(shifts))(*[int(v) for v in shifts])
    lib().ptc_pool_level_counts(ptr(code0.contiguous()), ptr(order0.contiguous()), code0.numel(), int(batch_shift), int(n_batch),
                                ctypes.cast(arr, ctypes.c_void_p), len(shifts), ptr(counts), stream_ptr())
    return counts


def pool_maps(code0: torch.Tensor, order0: torch.Tensor, shift: int, n_cluster: Optional[int] = None):
    """cluster (= pooling_inverse), idx_ptr, head for SerializedPooling (ptv3m1:383-396).
    One host sync (the number of clusters sizes the outputs, as torch.unique does in the reference) unless the caller
    already knows `n_cluster` (pool_level_counts)."""
    require_cuda(code0, order0)
    code0 = code0.contiguous()
    order0 = order0.contiguous()
    n = code0.numel()
    dev = code0.device
    cluster = torch.empty(n, dtype=torch.int64, device=dev)
    ncl = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = lib().ptc_pool_maps_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    lib().ptc_pool_maps_count(ptr(code0), ptr(order0), n, int(shift), ptr(cluster), ptr(ncl), ptr(ws), nbytes,
                              stream_ptr())
    if n_cluster is None:
        n_cluster = int(ncl.item())
    idx_ptr = torch.empty(n_cluster + 1, dtype=torch.int64, device=dev)
    head = torch.empty(n_cluster, dtype=torch.int64, device=dev)
    lib().ptc_pool_maps_fill(ptr(order0), ptr(cluster), n, n_cluster, ptr(idx_ptr), ptr(head), stream_ptr())
    return cluster, idx_ptr, head


def pool_child_codes(code: torch.Tensor, head: torch.Tensor, shift: int) -> torch.Tensor:
    require_cuda(code, head)
    code = code.contiguous()
    head = head.contiguous()
    k, n = code.shape
    nc = head.numel()
    out = torch.empty((k, nc), dtype=torch.int64, device=code.device)
    lib().ptc_pool_child_codes(ptr(code), n, k, ptr(head), nc, int(shift), ptr(out), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------
# voxelisation (GridSample front end)
# ------------------------------------------------------------------------------------------------
def voxel_keys(coord: torch.Tensor, grid_size: float):
    """floor(coord / grid_size) (float64 division), min-shifted, and the FNV-64 key of every point
    (pointcept/datasets/transform.py:867-875,997-1011) -> (grid_coord [N,3] i64, min_coord [3] i64, key [N] i64)."""
    require_cuda(coord)
    if coord.dtype != torch.float32 or coord.dim() != 2 or coord.shape[1] != 3:
        raise PtcoreError("coord must be float32 [N,3]")
    c = coord.contiguous()
    n = c.shape[0]
    grid = torch.empty((n, 3), dtype=torch.int64, device=c.device)
    mn = torch.empty(3, dtype=torch.int64, device=c.device)
    key = torch.empty(n, dtype=torch.int64, device=c.device)
    lib().ptc_voxel_keys(ptr(c), n, float(grid_size), ptr(grid), ptr(mn), ptr(key), stream_ptr())
    return grid, mn, key


# ------------------------------------------------------------------------------------------------
# pointops subset
# ------------------------------------------------------------------------------------------------
def _xyz(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise PtcoreError(f"{name} must be float32 [N,3]")
    return t.contiguous()


def knn_query(nsample: int, xyz, offset, new_xyz, new_offset):
    """-> (idx [m, nsample] int32, dist [m, nsample] fp32), libs/pointops/functions/query.py:7-26."""
    require_cuda(xyz, offset, new_xyz, new_offset)
    x, q = _xyz(xyz, "xyz"), _xyz(new_xyz, "new_xyz")
    off, noff = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    if off.numel() != noff.numel() or off.numel() == 0:
        raise PtcoreError("offset / new_offset must list the same (non-zero) number of scenes")
    m = q.shape[0]
    idx = torch.empty((m, nsample), dtype=torch.int32, device=x.device)
    dist = torch.empty((m, nsample), dtype=torch.float32, device=x.device)
    lib().ptc_knn_query(ptr(x), ptr(off), ptr(q), ptr(noff), off.numel(), x.shape[0], m, int(nsample), ptr(idx), ptr(dist),
                        stream_ptr())
    return idx, dist


def ball_query(nsample: int, max_radius: float, min_radius: float, xyz, offset, new_xyz, new_offset, order=None):
    """-> (idx [m, nsample] int32 (-1 = none), dist [m, nsample] fp32 (1e5 = none)), libs/pointops/functions/query.py:29-113.
    order = None: ball_query (sorted by distance, uniformly sub-sampled); order = int32 permutation of every scene's points:
    random_ball_query (first nsample in-range points in that order)."""
    require_cuda(xyz, offset, new_xyz, new_offset, order)
    if not float(min_radius) < float(max_radius):
        raise PtcoreError("min_radius must be smaller than max_radius")      # query.py:45,93
    x, q = _xyz(xyz, "xyz"), _xyz(new_xyz, "new_xyz")
    off, noff = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    if off.numel() != noff.numel() or off.numel() == 0:
        raise PtcoreError("offset / new_offset must list the same (non-zero) number of scenes")
    if order is not None:
        order = order.to(torch.int32).contiguous()
        if order.numel() != x.shape[0]:
            raise PtcoreError("order must be a permutation of the source points")
    m = q.shape[0]
    idx = torch.empty((m, nsample), dtype=torch.int32, device=x.device)
    d2 = torch.empty((m, nsample), dtype=torch.float32, device=x.device)
    lib().ptc_ball_query(ptr(x), ptr(off), ptr(q), ptr(noff), ptr(order), off.numel(), x.shape[0], m, int(nsample), float(min_radius),
                         float(max_radius), ptr(idx), ptr(d2), stream_ptr())
    return idx, torch.sqrt(d2)


def farthest_point_sampling(xyz, offset, new_offset):
    """-> idx [new_offset[-1]] int32, libs/pointops/functions/sampling.py:7-24 (one host sync for the output size)."""
    require_cuda(xyz, offset, new_offset)
    x = _xyz(xyz, "xyz")
    off, noff = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    if off.numel() != noff.numel() or off.numel() == 0:
        raise PtcoreError("offset / new_offset must list the same (non-zero) number of scenes")
    idx = torch.zeros(int(noff[-1].item()), dtype=torch.int32, device=x.device)
    tmp = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    lib().ptc_farthest_point_sampling(ptr(x), ptr(off), ptr(noff), off.numel(), x.shape[0], ptr(tmp), ptr(idx), stream_ptr())
    return idx


# ------------------------------------------------------------------------------------------------
# edge-list operators of libs/pointops (grouping / interpolation / aggregation / subtraction): csrc/pointops_edges.hip
# ------------------------------------------------------------------------------------------------
def _f32_rows(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise PtcoreError(f"{name} must be float32 (the reference kernels are fp32-only)")
    return t.contiguous()


def _edge_idx(idx: torch.Tensor):
    if idx.dim() != 2:
        raise PtcoreError("idx must be [m, nsample]")
    return idx.to(torch.int32).contiguous()


def edge_rows(mode: int, src, a, idx, out=None, out_col0: int = 0):
    """Per-edge rows (GROUP src[j], SUB a[t] - src[j], REL src[j] - a[t] with zeros for empty slots) -> out [m, nsample, c], or written
    into the column window [out_col0, out_col0 + c) of a caller's wider `out` [m, nsample, width]."""
    require_cuda(src, a, idx, out)
    src, idx = _f32_rows(src, "src"), _edge_idx(idx)
    a = None if a is None else _f32_rows(a, "a")
    m, ns = idx.shape
    c = src.shape[1]
    if out is None:
        out = torch.empty((m, ns, c), dtype=torch.float32, device=src.device)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape[:2] != (m, ns):
        raise PtcoreError("edge_rows: out must be a contiguous fp32 [m, nsample, width] tensor")
    lib().ptc_edge_rows_fwd(int(mode), ptr(src), ptr(a), ptr(idx), m * ns, ns, c, src.shape[0], ptr(out), out.shape[2], int(out_col0),
                            stream_ptr())
    return out


def edge_reduce(mode: int, src, pos, w, idx, m: int, nsample: int, c: int, w_c: int = 1, pos_stride: int = 0, pos_col0: int = 0):
    """Per-target sums over the nsample edges of a row -> [m, c] (INTERP interpolation, AGG aggregation, POS plain row sums of `pos`)."""
    require_cuda(src, pos, w, idx)
    out = torch.empty((m, c), dtype=torch.float32, device=(pos if src is None else src).device)
    n_src = 0 if src is None else src.shape[0]
    lib().ptc_edge_reduce_fwd(int(mode), ptr(src), ptr(pos), int(pos_stride), int(pos_col0), ptr(w), ptr(idx), int(m), int(nsample),
                              int(c), int(w_c), n_src, ptr(out), stream_ptr())
    return out


class EdgeCSR:
    """The edges of idx [m, nsample] sorted by source row (stable: ascending edge index inside a row) + the CSR pointer: what the
    segmented, atomics-free gradients of the gathered operands walk.  Built on first use: the engine's radix sort over
    bit_length(n_src) bits and two small kernels."""

    def __init__(self, idx: torch.Tensor, n_src: int):
        require_cuda(idx)
        self.idx, self.n_src = _edge_idx(idx), int(n_src)
        self.order = self.indptr = None

    def build(self):
        if self.order is None:
            e = self.idx.numel()
            keys = torch.empty(e, dtype=torch.int64, device=self.idx.device)
            lib().ptc_edge_csr_keys(ptr(self.idx), e, self.n_src, ptr(keys), stream_ptr())
            self.order, _ = sort_keys(keys, 0, max(1, int(self.n_src).bit_length()), want_inverse=False) if e else (keys, None)
            self.indptr = torch.empty(self.n_src + 1, dtype=torch.int64, device=self.idx.device)
            lib().ptc_edge_csr_ptr(ptr(keys), ptr(self.order), e, self.n_src, ptr(self.indptr), stream_ptr())
        return self


def edge_scatter_bwd(mode: int, csr: EdgeCSR, g, w, nsample: int, c: int, w_c: int = 1, g_col0: int = 0):
    """grad of the gathered operand [n_src, c]: segmented sum over the edges of every source row (fixed order, no atomics).
    g: [E or m, width] rows (fp32, contiguous); the window [g_col0, g_col0 + c) of each row is summed."""
    require_cuda(g, w)
    csr.build()
    g = _f32_rows(g, "grad").reshape(-1, g.shape[-1])
    out = torch.empty((csr.n_src, c), dtype=torch.float32, device=g.device)
    lib().ptc_edge_scatter_bwd(int(mode), ptr(csr.order), ptr(csr.indptr), ptr(g), g.shape[1], int(g_col0), ptr(w), int(nsample), int(c),
                               int(w_c), csr.n_src, ptr(out), stream_ptr())
    return out


def pair_dot_weighted(a, b, w, ia, ib) -> torch.Tensor:
    """out[m, g] = sum_c a[ia[m], g, c] b[ib[m], g, c] (w[c] | 1); a [n_a, g, c], b [n_b, g, c] fp32, ia / ib [m] int32"""
    require_cuda(a, b, w, ia, ib)
    a, b = a.float().contiguous(), b.float().contiguous()
    if a.dim() != 3 or b.dim() != 3 or a.shape[1:] != b.shape[1:]:
        raise PtcoreError(f"pair_dot_weighted: rows must be [n, g, c], got {tuple(a.shape)} / {tuple(b.shape)}")
    ia, ib = ia.reshape(-1).to(torch.int32).contiguous(), ib.reshape(-1).to(torch.int32).contiguous()
    if ia.numel() != ib.numel():
        raise PtcoreError("pair_dot_weighted: index lists differ in length")
    w = None if w is None else w.float().contiguous()
    _, g, c = a.shape
    if w is not None and w.numel() != c:
        raise PtcoreError(f"pair_dot_weighted: weight has {w.numel()} entries, rows have {c} channels")
    out = torch.empty((ia.numel(), g), dtype=torch.float32, device=a.device)
    lib().ptc_pair_dot_weighted(ptr(a), ptr(b), ptr(w), ptr(ia), ptr(ib), ia.numel(), a.shape[0], b.shape[0], g, c, ptr(out),
                                stream_ptr())
    return out


def pair_segment_sum(s, b, w, self_rows, csr: "EdgeCSR", oidx, want_prod: bool = False):
    """A[n, g, c] = sum over the pairs e of row n (csr: the pairs by that row, ascending) of s[e, g] b[oidx[e], g, c];
    -> (A * (w | 1), self_rows * A | None).  s [m, g], b [n_b, g, c] fp32, oidx [m] int32."""
    require_cuda(s, b, w, self_rows, oidx)
    csr.build()
    s, b = s.float().contiguous(), b.float().contiguous()
    oidx = oidx.reshape(-1).to(torch.int32).contiguous()
    _, g, c = b.shape
    if s.shape != (oidx.numel(), g):
        raise PtcoreError(f"pair_segment_sum: coefficients {tuple(s.shape)} for {oidx.numel()} pairs of {g} groups")
    w = None if w is None else w.float().contiguous()
    out = torch.empty((csr.n_src, g, c), dtype=torch.float32, device=b.device)
    prod = None
    if want_prod:
        self_rows = self_rows.float().contiguous()
        if tuple(self_rows.shape) != (csr.n_src, g, c):
            raise PtcoreError("pair_segment_sum: self rows do not match the output")
        prod = torch.empty_like(out)
    lib().ptc_pair_segment_sum(ptr(s), ptr(b), ptr(w), ptr(self_rows) if want_prod else None, ptr(csr.order), ptr(csr.indptr), ptr(oidx),
                               csr.n_src, b.shape[0], g, c, ptr(out), ptr(prod), stream_ptr())
    return out, prod


def aggregation_edge_bwd(src, pos, w, idx, g):
    """-> (grad_position [m, nsample, c], grad_weight [m, nsample, w_c]) of libs/pointops aggregation."""
    require_cuda(src, pos, w, idx, g)
    m, ns, c = pos.shape
    gp, gw = torch.empty_like(pos), torch.empty_like(w)
    lib().ptc_aggregation_edge_bwd(ptr(src), ptr(pos), ptr(w), ptr(idx), ptr(g), m, ns, c, w.shape[-1], src.shape[0], ptr(gp), ptr(gw),
                                   stream_ptr())
    return gp, gw


# ------------------------------------------------------------------------------------------------
# rows
# ------------------------------------------------------------------------------------------------
def gather_rows(src: torch.Tensor, idx: torch.Tensor, idx2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = src[idx[i]] (+ src[idx2[i]] where idx2[i] >= 0); idx[i] < 0 -> zeros."""
    require_cuda(src, idx, idx2)
    if src.dim() != 2:
        raise PtcoreError("gather_rows expects [N,C] features")
    src = src.contiguous()
    idx = idx.to(torch.int64).contiguous()
    if idx2 is not None:
        idx2 = idx2.to(torch.int64).contiguous()
    n_out, c = idx.numel(), src.shape[1]
    out = torch.empty((n_out, c), dtype=src.dtype, device=src.device)
    lib().ptc_gather_rows(ptr(src), src.shape[0], ptr(idx), ptr(idx2), n_out, c, dtype_code(src), ptr(out),
                          stream_ptr())
    return out


def gather_rows_add_supported(src: torch.Tensor, addend: torch.Tensor) -> bool:
    return (src.dim() == 2 and addend.dim() == 2 and src.dtype == addend.dtype and src.shape[1] == addend.shape[1]
            and src.dtype in _DT and bool(_ask("ptc_gather_rows_add_supported", int(src.shape[1]), _DT[src.dtype])))


def gather_rows_add(src: torch.Tensor, idx: torch.Tensor, addend: torch.Tensor) -> torch.Tensor:
    """out[i] = addend[i] + src[idx[i]] in one pass (SerializedUnpooling, ptv3m1:478)."""
    require_cuda(src, idx, addend)
    if not gather_rows_add_supported(src, addend) or addend.shape[0] != idx.numel():
        raise PtcoreError(f"gather_rows_add: src {tuple(src.shape)} {src.dtype}, addend {tuple(addend.shape)} {addend.dtype}, idx {tuple(idx.shape)}")
    src, addend = src.contiguous(), addend.contiguous()
    idx = idx.to(torch.int64).contiguous()
    out = torch.empty_like(addend)
    lib().ptc_gather_rows_add(ptr(src), src.shape[0], ptr(idx), ptr(addend), idx.numel(), src.shape[1], dtype_code(src), ptr(out), stream_ptr())
    return out


def segment_csr_fwd(src: torch.Tensor, perm: Optional[torch.Tensor], indptr: torch.Tensor, reduce: str):
    """out[s] = reduce_{r in [indptr[s], indptr[s+1])} src[perm[r]]; returns (out, arg|None)."""
    require_cuda(src, perm, indptr)
    src = src.contiguous()
    indptr = indptr.to(torch.int64).contiguous()
    if perm is not None:
        perm = perm.to(torch.int64).contiguous()
    n_seg, c = indptr.numel() - 1, src.shape[1]
    out = torch.empty((n_seg, c), dtype=src.dtype, device=src.device)
    arg = torch.empty((n_seg, c), dtype=torch.int32, device=src.device) if reduce in ("max", "min") else None
    lib().ptc_segment_csr_fwd(ptr(src), ptr(perm), ptr(indptr), n_seg, c, dtype_code(src),
                              _lib.REDUCE_CODES[reduce], ptr(out), ptr(arg), stream_ptr())
    return out, arg


def segment_csr_bwd(grad_out: torch.Tensor, perm: Optional[torch.Tensor], indptr: torch.Tensor,
                    arg: Optional[torch.Tensor], n_src: int, reduce: str, covers_all: bool = False) -> torch.Tensor:
    require_cuda(grad_out, perm, indptr, arg)
    grad_out = grad_out.contiguous()
    n_seg, c = indptr.numel() - 1, grad_out.shape[1]
    # rows outside every segment (none when perm is a full permutation) must read as zero
    covered = int(n_src)
    alloc = torch.empty if covers_all else torch.zeros      # covers_all: every row belongs to a segment and gets written
    gsrc = alloc((covered, c), dtype=grad_out.dtype, device=grad_out.device)
    lib().ptc_segment_csr_bwd(ptr(grad_out), ptr(perm), ptr(indptr), ptr(arg), n_seg, covered, c,
                              dtype_code(grad_out), _lib.REDUCE_CODES[reduce], ptr(gsrc), stream_ptr())
    return gsrc


# ------------------------------------------------------------------------------------------------
# rulebooks
# ------------------------------------------------------------------------------------------------
VOX_MAX = 1 << _K["PTC_VOX_BITS"]
BATCH_MAX = _K["PTC_VOX_BATCH_MAX"]


def check_coord_range(coord_max_host, batch_size: int, spatial_shape=None) -> None:
    """The voxel hash packs (batch, x, y, z) into 10 + 3 x PTC_VOX_BITS bits (csrc/voxel_hash.h): coordinates outside [0, VOX_MAX) --
    ptc_coord_max reports a negative coordinate as a negative maximum -- or outside the declared spatial_shape, or more
    than BATCH_MAX batch items, would alias other voxels' keys and give silently wrong neighbour maps.  Host integers
    only (they ride in the one host sync of the forward): no device work."""
    for a, m in enumerate(coord_max_host):
        m = int(m)
        if m < 0 or m >= VOX_MAX:
            raise PtcoreError(f"grid_coord axis {a}: coordinates must lie in [0, {VOX_MAX}) (max reported {m}; negative = a negative "
                              "coordinate in the input)")
        if spatial_shape is not None and m >= int(spatial_shape[a]):
            raise PtcoreError(f"grid_coord axis {a}: maximum {m} outside the declared spatial_shape {list(spatial_shape)}")
    if int(batch_size) > BATCH_MAX:
        raise PtcoreError(f"batch size {batch_size} exceeds the {BATCH_MAX} batch items the voxel key can hold")


class HashTable:
    def __init__(self, indices: torch.Tensor):
        require_cuda(indices)
        if indices.dtype != torch.int32 or indices.dim() != 2 or indices.shape[1] != 4:
            raise PtcoreError("indices must be int32 [N,4] (batch,x,y,z)")
        self.indices = indices.contiguous()
        n = self.indices.shape[0]
        self.size = int(lib().ptc_hash_table_size(n))            # buckets of 2x2x2 voxels, 64 bytes each
        self.nbytes = int(lib().ptc_hash_table_bytes(n))
        self.buf = torch.empty(self.nbytes // 8, dtype=torch.int64, device=indices.device)   # torch allocations are >= 256 B aligned
        lib().ptc_hash_build(ptr(self.indices), n, ptr(self.buf), self.nbytes, stream_ptr())


def rulebook_subm(indices: torch.Tensor, ksize: int, table: Optional[HashTable] = None) -> torch.Tensor:
    """Gather table nbr [ksize^3, N] int32 of a submanifold convolution."""
    if table is None:
        table = HashTable(indices)
    ind = table.indices
    n = ind.shape[0]
    nbr = torch.empty((ksize ** 3, n), dtype=torch.int32, device=ind.device)
    lib().ptc_rulebook_subm(ptr(ind), n, int(ksize), ptr(table.buf), table.nbytes, ptr(nbr), stream_ptr())
    return nbr


BLOCK_BM, BLOCK_HCAP = _K["PTC_BLOCK_BM"], _K["PTC_BLOCK_HCAP"]


class BlockTables:
    """Block-local form of a submanifold 3^3 gather table `nbr` (csrc/blocks.hip): per block of 128 consecutive rows the ascending list
    of distinct input rows (`hid` [n_blocks, hcap], `hcnt` [n_blocks]; -1 = does not fit) and the uint16 tables `tab`
    [2, n_blocks, 28, 32, 4] of LDS byte offsets of those rows (0: 64-channel rows, 1: 32-channel rows; include/ptcore.h).  Consumed by
    spconv_fwd(..., blk=...) (csrc/conv7.h)."""

    def __init__(self, nbr: torch.Tensor, bm: int = BLOCK_BM, hcap: int = BLOCK_HCAP):
        require_cuda(nbr)
        if nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != 27:
            raise PtcoreError("nbr must be int32 [27, n]")
        self.nbr = nbr.contiguous()
        kv, n = self.nbr.shape
        self.bm, self.hcap = int(bm), int(hcap)
        nblk = max(1, (n + self.bm - 1) // self.bm)
        dev = nbr.device
        self.tab = torch.empty(int(lib().ptc_rulebook_blocks_tab_bytes(n)) // 2, dtype=torch.int16, device=dev).view(2, nblk, 28, 32, 4)
        self.hid = torch.empty((nblk, self.hcap), dtype=torch.int32, device=dev)
        self.hcnt = torch.empty(nblk, dtype=torch.int32, device=dev)
        self.n_overflow = torch.empty(1, dtype=torch.int32, device=dev)
        lib().ptc_rulebook_blocks(ptr(self.nbr), kv, n, self.bm, self.hcap, ptr(self.tab), ptr(self.hid), ptr(self.hcnt),
                                  ptr(self.n_overflow), stream_ptr())


def block_plan(c_in: int, c_out: int, kv: int, dtype: torch.dtype, n_rows: int = 1 << 30):
    """(bm, hcap) of the block-local tables for this shape, or None when it stays on the global-gather kernels: what the weight gradient
    takes (wgrad7_supported, csrc/wgrad7.h: conv7's shapes and the sliced wider ones; conv7 / conv8 take a subset: BlockProvider.get)."""
    return (BLOCK_BM, BLOCK_HCAP) if _blk_takes("PTC_CONSUMER_WGRAD7", c_in, c_out, kv, dtype, n_rows) else None


def _blk_takes(consumer: str, c_in: int, c_out: int, kv: int, dtype: torch.dtype, n_rows: int) -> bool:
    """whether `consumer` (enum ptc_blk_consumer) takes such tables of n_rows rows: the launch paths' predicates, asked once per shape"""
    return dtype in _DT and 0 <= _ask("ptc_spconv_blk_min_rows", _K[consumer], int(kv), int(c_in), int(c_out), _DT[dtype]) <= n_rows


class BlockProvider:
    """lazily built BlockTables of ONE gather table; lives next to the table in the rulebook cache."""

    def __init__(self, nbr: torch.Tensor):
        self.nbr = nbr
        self.tables = {}

    def get(self, c_in: int, c_out: int, dtype: torch.dtype, conv: bool = False):
        """conv=True: asked by a forward / input-gradient convolution -- only the shapes conv7 or conv8 would take (the library's answer,
        PTC_CONV8 included) get tables there; the sliced weight gradient of the other shapes asks with conv=False from the backward, so
        inference, eval and PTC_WGRAD_BLK=0 never pay the table build (one launch + ~112 B per row) for a kernel that cannot use it."""
        if not self.nbr.is_cuda:
            return None
        kv, n = self.nbr.shape
        plan = block_plan(c_in, c_out, kv, dtype, n)
        if plan is None or (conv and not (_blk_takes("PTC_CONSUMER_CONV7", c_in, c_out, kv, dtype, n)
                                          or _blk_takes("PTC_CONSUMER_CONV8", c_in, c_out, kv, dtype, n))):
            return None
        t = self.tables.get(plan)
        if t is None:
            t = self.tables[plan] = BlockTables(self.nbr, *plan)
        return t


def rulebook_down(indices: torch.Tensor, coord_bits: int, batch_bits: int):
    """k=2,s=2 strided conv maps: out_indices [M,4] i32, nbr_down [8,M] i32, nbr_up [8,N] i32."""
    require_cuda(indices)
    ind = indices.contiguous()
    n = ind.shape[0]
    dev = ind.device
    out_of_in = torch.empty(n, dtype=torch.int32, device=dev)
    n_out_dev = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = lib().ptc_rulebook_down_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    lib().ptc_rulebook_down_count(ptr(ind), n, int(coord_bits), int(batch_bits), ptr(out_of_in), ptr(n_out_dev),
                                  ptr(ws), nbytes, stream_ptr())
    n_out = int(n_out_dev.item())
    out_indices = torch.empty((n_out, 4), dtype=torch.int32, device=dev)
    nbr_down = torch.empty((8, n_out), dtype=torch.int32, device=dev)
    nbr_up = torch.empty((8, n), dtype=torch.int32, device=dev)
    lib().ptc_rulebook_down_fill(ptr(ind), n, ptr(out_of_in), n_out, ptr(out_indices), ptr(nbr_down), ptr(nbr_up),
                                 stream_ptr())
    return out_indices, nbr_down, nbr_up


# ------------------------------------------------------------------------------------------------
# sparse conv compute
# ------------------------------------------------------------------------------------------------
def spconv_fwd(feat: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
               nbr: Optional[torch.Tensor], blk: Optional["BlockTables"] = None) -> torch.Tensor:
    """out[o] = bias + sum_k W[:,k,:] . feat[nbr[k][o]].  weight [C_out, kv, C_in] in feat.dtype,
    bias fp32.  C_in % 8 == 0 and C_out % 16 == 0 (callers pad).  nbr=None (kv == 1): identity
    table, i.e. the dense row-wise GEMM out = feat @ W[:,0,:]^T + bias.  blk = BlockTables of `nbr`: the
    LDS-staged kernel (same result up to the fp32 rounding of its summation order)."""
    require_cuda(feat, weight, bias, nbr)
    feat = feat.contiguous()
    weight = weight.contiguous()
    if weight.dtype != feat.dtype:
        raise PtcoreError("weight dtype must match feature dtype")
    c_out, kv, c_in = weight.shape
    if nbr is not None:
        nbr = nbr.contiguous()
        if nbr.shape[0] != kv or nbr.dtype != torch.int32:
            raise PtcoreError(f"table mismatch: weight {tuple(weight.shape)} nbr {tuple(nbr.shape)} {nbr.dtype}")
    elif kv != 1:
        raise PtcoreError("nbr=None needs kv == 1")
    if feat.shape[1] != c_in:
        raise PtcoreError(f"shape mismatch: feat {tuple(feat.shape)} weight {tuple(weight.shape)}")
    if bias is not None:
        bias = bias.to(torch.float32).contiguous()
    n_out = nbr.shape[1] if nbr is not None else feat.shape[0]
    out = torch.empty((n_out, c_out), dtype=feat.dtype, device=feat.device)
    if blk is not None and nbr is not None:
        if blk.nbr.data_ptr() != nbr.data_ptr() or tuple(blk.nbr.shape) != tuple(nbr.shape):
            raise PtcoreError("blk was built from another gather table")
        nbytes = _ask("ptc_spconv_fwd_blk_workspace_bytes", 0, kv, c_in, c_out)       # the wide kernel's fragment-ordered weights; n_out is ignored
        ws = torch.empty(nbytes, dtype=torch.uint8, device=feat.device) if nbytes else None
        lib().ptc_spconv_fwd_blk(ptr(feat), feat.shape[0], ptr(weight), ptr(bias), ptr(nbr), ptr(blk.tab), ptr(blk.hid),
                                 ptr(blk.hcnt), blk.bm, blk.hcap, n_out, kv, c_in, c_out, dtype_code(feat), ptr(out),
                                 ptr(ws), nbytes, stream_ptr())
        return out
    lib().ptc_spconv_fwd(ptr(feat), feat.shape[0], ptr(weight), ptr(bias), ptr(nbr), n_out, kv, c_in, c_out,
                         dtype_code(feat), ptr(out), stream_ptr())
    return out


def spconv_wgrad(feat: torch.Tensor, dout: torch.Tensor, nbr: Optional[torch.Tensor], want_bias: bool = False,
                 blk: Optional["BlockTables"] = None):
    """dw [C_out, kv, C_in] fp32 = sum_o dout[o]^T (x) feat[nbr[k][o]]  (nbr=None: identity, kv=1);
    with want_bias also dbias [C_out] fp32 = column sums of dout (fused).  Returns dw or (dw, dbias).  blk = BlockTables of `nbr`
    (and no bias gradient): the block-staged, accumulator-stationary kernel (csrc/wgrad7.h; same result up to the fp32 rounding of
    its summation order)."""
    require_cuda(feat, dout, nbr)
    feat = feat.contiguous()
    dout = dout.contiguous()
    if feat.dtype != dout.dtype:
        raise PtcoreError("feat / dout dtype mismatch")
    if nbr is not None:
        nbr = nbr.contiguous()
        kv, n_out = nbr.shape
    else:
        kv, n_out = 1, dout.shape[0]
    c_in, c_out = feat.shape[1], dout.shape[1]
    dw = torch.empty((c_out, kv, c_in), dtype=torch.float32, device=feat.device)
    if blk is not None and nbr is not None and not want_bias:
        if blk.nbr.data_ptr() != nbr.data_ptr() or tuple(blk.nbr.shape) != tuple(nbr.shape):
            raise PtcoreError("blk was built from another gather table")
        nbytes = lib().ptc_spconv_wgrad_blk_workspace_bytes(n_out, kv, c_in, c_out)
        ws = _ws(nbytes, feat.device)
        lib().ptc_spconv_wgrad_blk(ptr(feat), feat.shape[0], ptr(dout), ptr(nbr), ptr(blk.tab), ptr(blk.hid), ptr(blk.hcnt),
                                   ptr(blk.n_overflow), blk.bm, blk.hcap, n_out, kv, c_in, c_out, dtype_code(feat), ptr(dw), ptr(ws),
                                   nbytes, stream_ptr())
        return dw
    db = torch.empty(c_out, dtype=torch.float32, device=feat.device) if want_bias else None
    nbytes = lib().ptc_spconv_wgrad_workspace_bytes(n_out, kv, c_in, c_out)
    ws = _ws(nbytes, feat.device)
    lib().ptc_spconv_wgrad(ptr(feat), feat.shape[0], ptr(dout), ptr(nbr), n_out, kv, c_in, c_out,
                           dtype_code(feat), ptr(dw), ptr(db), ptr(ws), nbytes, stream_ptr())
    return (dw, db) if want_bias else dw


# ------------------------------------------------------------------------------------------------
# evaluation tail: arg-max + inverse gather + three class histograms in one pass
# ------------------------------------------------------------------------------------------------
def seg_eval_hist(logits: Optional[torch.Tensor], target: torch.Tensor, k: int, ignore_index: int = -1,
                  inverse: Optional[torch.Tensor] = None, pred: Optional[torch.Tensor] = None):
    """(area_intersection, area_union, area_target), each int64 [k]: pointcept/utils/misc.py:57-69 applied to
    pred = logits.max(1)[1][inverse] (pointcept/engines/hooks/evaluator.py:139-147), or to given predictions."""
    require_cuda(logits, target, inverse, pred)
    if (logits is None) == (pred is None):
        raise PtcoreError("give logits or pred")
    target = target.reshape(-1).to(torch.int64).contiguous()
    m = target.numel()
    hist = torch.empty((3, int(k)), dtype=torch.int64, device=target.device)
    if pred is not None:
        pred = pred.reshape(-1).to(torch.int64).contiguous()
        if pred.numel() != m:
            raise PtcoreError("pred / target size mismatch")            # misc.py:60
        lib().ptc_seg_eval_hist(0, 0, 0, 0, ptr(pred), 0, ptr(target), m, 0, int(k), int(ignore_index), ptr(hist), stream_ptr())
    else:
        if logits.dim() != 2 or logits.stride(1) != 1:
            raise PtcoreError("logits must be [N, C] with unit column stride")
        if inverse is not None:
            inverse = inverse.reshape(-1).to(torch.int64).contiguous()
            if inverse.numel() != m:
                raise PtcoreError("inverse / target size mismatch")
        elif logits.shape[0] != m:
            raise PtcoreError("logits / target size mismatch")
        lib().ptc_seg_eval_hist(ptr(logits), dtype_code(logits), logits.stride(0), logits.shape[1], 0, ptr(inverse), ptr(target), m,
                                logits.shape[0], int(k), int(ignore_index), ptr(hist), stream_ptr())
    return hist[0], hist[1] + hist[2] - hist[0], hist[2]


# ------------------------------------------------------------------------------------------------
# 3-axis rotary embedding (libs/pointrope)
# ------------------------------------------------------------------------------------------------
def rope3d_(tokens: torch.Tensor, positions: torch.Tensor, base: float, fwd: float) -> torch.Tensor:
    """in place on tokens [..., H, D] (contiguous, D % 6 == 0) with positions [..., 3] int64 (libs/pointrope/kernels.cu:19-100)"""
    require_cuda(tokens, positions)
    if tokens.dim() < 3 or not tokens.is_contiguous():
        raise PtcoreError("tokens must be contiguous [..., H, D]")       # kernels.cu:83: "tokens are not contiguous"
    if positions.dtype != torch.int64 or not positions.is_contiguous() or positions.shape[-1] != 3:
        raise PtcoreError("positions must be contiguous int64 [..., 3]")
    H, D = tokens.shape[-2], tokens.shape[-1]
    n = tokens.numel() // (H * D) if H * D > 0 else 0
    if positions.numel() != 3 * n:
        raise PtcoreError(f"positions {tuple(positions.shape)} do not match tokens {tuple(tokens.shape)}")
    lib().ptc_rope3d(ptr(tokens), dtype_code(tokens), ptr(positions), n, H, D, float(base), float(fwd), stream_ptr())
    return tokens


def rope3d_xyz(qkv: torch.Tensor, xyz: torch.Tensor, inv_freq: torch.Tensor, rot_slabs: int, sign: float,
               out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """PT-v3m3 Point3DRoPE on packed rows: qkv [n, S, H, D] -> same shape in `out_dtype` (default: qkv's), the first `rot_slabs`
    slabs rotated with xyz [n, 3] fp32 and inv_freq [D/6] fp32, the rest converted (point_transformer_v3m3_utonia.py:43-102,274-323).
    sign = +1 forward / -1 gradient."""
    require_cuda(qkv, xyz, inv_freq)
    if qkv.dim() != 4 or not qkv.is_contiguous():
        raise PtcoreError("rope3d_xyz: qkv must be contiguous [n, slabs, H, D]")
    n, S, H, D = qkv.shape
    if D % 6 != 0:
        raise PtcoreError(f"rope3d_xyz: head dim {D} must be a multiple of 6")
    if xyz.dtype != torch.float32 or tuple(xyz.shape) != (n, 3) or not xyz.is_contiguous():
        raise PtcoreError("rope3d_xyz: xyz must be contiguous fp32 [n, 3]")
    if inv_freq.dtype != torch.float32 or inv_freq.numel() != D // 6 or not inv_freq.is_contiguous():
        raise PtcoreError(f"rope3d_xyz: inv_freq must be contiguous fp32 [{D // 6}]")
    out = torch.empty(qkv.shape, dtype=out_dtype or qkv.dtype, device=qkv.device)
    lib().ptc_rope3d_xyz(ptr(qkv), dtype_code(qkv), ptr(out), dtype_code(out), ptr(xyz), ptr(inv_freq), n, S, int(rot_slabs), H, D,
                         float(sign), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------
# layer norm
# ------------------------------------------------------------------------------------------------
def layer_norm_supported(c: int) -> bool:
    """the power-of-two instances (C = 32 .. 512): the widths the GEMM-epilogue joints and the Block executor are built for"""
    return lib().ptc_layer_norm_supported(int(c)) == 1


def layer_norm_joint_available(c: int) -> bool:
    """the fused residual joints (add_norm_fwd / _bwd) take this width: every width LayerNorm takes (round 5: generic even widths too)"""
    return lib().ptc_layer_norm_supported(int(c)) != 0


def layer_norm_available(c: int) -> bool:
    """layer_norm_fwd / _bwd take this width (the instances above, or the wave-per-row form: any even C <= 1024)"""
    return lib().ptc_layer_norm_supported(int(c)) != 0


def layer_norm_fwd(x: torch.Tensor, gamma, beta, eps: float, out_dtype: torch.dtype):
    """y [N,C] (out_dtype), mean [N], rstd [N] (fp32).  gamma / beta fp32 or None."""
    require_cuda(x, gamma, beta)
    x = x.contiguous()
    n, c = x.shape
    g = None if gamma is None else gamma.to(torch.float32).contiguous()
    b = None if beta is None else beta.to(torch.float32).contiguous()
    y = torch.empty((n, c), dtype=out_dtype, device=x.device)
    mean = torch.empty(n, dtype=torch.float32, device=x.device)
    rstd = torch.empty(n, dtype=torch.float32, device=x.device)
    lib().ptc_layer_norm_fwd(ptr(x), n, c, dtype_code(x), ptr(g), ptr(b), float(eps), ptr(y), _DT[out_dtype],
                             ptr(mean), ptr(rstd), stream_ptr())
    return y, mean, rstd


def layer_norm_bwd(dy: torch.Tensor, x: torch.Tensor, mean, rstd, gamma, want_affine: bool = True):
    """dx (x.dtype), dgamma, dbeta (fp32 or None)."""
    require_cuda(dy, x, mean, rstd, gamma)
    dy = dy.contiguous()
    x = x.contiguous()
    n, c = x.shape
    g = None if gamma is None else gamma.to(torch.float32).contiguous()
    dx = torch.empty_like(x)
    dg = torch.empty(c, dtype=torch.float32, device=x.device) if want_affine else None
    db = torch.empty(c, dtype=torch.float32, device=x.device) if want_affine else None
    nbytes = lib().ptc_layer_norm_bwd_workspace_bytes(n, c)
    ws = _ws(nbytes, x.device)
    lib().ptc_layer_norm_bwd(ptr(dy), dtype_code(dy), ptr(x), dtype_code(x), ptr(mean), ptr(rstd), ptr(g), n, c,
                             ptr(dx), ptr(dg), ptr(db), ptr(ws), nbytes, stream_ptr())
    return dx, dg, db


def add_norm_fwd(u, a, row_scale, norm_a, norm_b, y_dtype):
    """z = a + row_scale * f(u) (fp32), y = g(z) (y_dtype or None).  norm_a / norm_b: (gamma, beta, eps) or
    None (identity).  Returns (z, y, statA, statB)."""
    require_cuda(u, a, row_scale)
    u = u.contiguous()
    a = a.contiguous()
    if a.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise PtcoreError("add_norm: the residual operand `a` must be fp32, bf16 or f16")
    n, c = u.shape
    dev = u.device
    z = torch.empty((n, c), dtype=torch.float32, device=dev)
    y = torch.empty((n, c), dtype=y_dtype, device=dev) if y_dtype is not None else None
    st_a = torch.empty((2, n), dtype=torch.float32, device=dev) if norm_a is not None else None
    st_b = torch.empty((2, n), dtype=torch.float32, device=dev) if (norm_b is not None and y is not None) else None
    ga, ba, ea = norm_a if norm_a is not None else (None, None, 0.0)
    gb, bb, eb = norm_b if norm_b is not None else (None, None, 0.0)
    rs = None if row_scale is None else row_scale.to(torch.float32).contiguous()
    lib().ptc_add_norm_fwd(ptr(u), dtype_code(u), ptr(a), dtype_code(a), ptr(rs), n, c, ptr(ga), ptr(ba), float(ea),
                           int(norm_a is not None), ptr(gb), ptr(bb), float(eb), int(norm_b is not None), ptr(z), ptr(y),
                           _DT[y_dtype] if y_dtype is not None else 0, ptr(st_a), ptr(st_b), stream_ptr())
    return z, y, st_a, st_b


def linear_joint_supported(c_in: int, c_out: int, dtype: torch.dtype) -> bool:
    return dtype in _DT and bool(lib().ptc_linear_joint_supported(int(c_in), int(c_out), _DT[dtype]))


def linear_joint_fwd(x, weight, bias, table, a, row_scale, norm_b, y_dtype, n_out=None):
    """z = a + row_scale * (x[table] @ weight^T + bias) (fp32), y = LN_B(z) | cast(z) -- a Linear of the Block with the residual joint behind
    it in its epilogue (csrc/fwd2_joint.h; bit-identical to spconv_fwd + add_norm_fwd).  weight [c_out, c_in] in x's 16-bit dtype, table
    None or the kv = 1 gather table [1, n_out] / [n_out] int32 (the inverse serialization table of `proj`), a [n_out, c_out] fp32.
    Returns (z, y, statB)."""
    require_cuda(x, weight, bias, table, a, row_scale)
    x, weight, a = x.contiguous(), weight.contiguous(), a.contiguous()
    c_out, c_in = weight.shape[0], weight.shape[-1]
    if a.dtype != torch.float32 or x.dtype != weight.dtype or not linear_joint_supported(c_in, c_out, x.dtype):
        raise PtcoreError("linear_joint_fwd: unsupported shape / dtype")
    n = int(a.shape[0]) if n_out is None else int(n_out)
    tab = None if table is None else table.reshape(-1).to(torch.int32).contiguous()
    dev = x.device
    z = torch.empty((n, c_out), dtype=torch.float32, device=dev)
    y = torch.empty((n, c_out), dtype=y_dtype, device=dev) if y_dtype is not None else None
    st_b = torch.empty((2, n), dtype=torch.float32, device=dev) if (norm_b is not None and y is not None) else None
    gb, bb, eb = norm_b if norm_b is not None else (None, None, 0.0)
    rs = None if row_scale is None else row_scale.to(torch.float32).contiguous()
    b = None if bias is None else bias.float().contiguous()
    lib().ptc_linear_joint_fwd(ptr(x), x.shape[0], ptr(weight), ptr(b), ptr(tab), n, c_in, c_out, dtype_code(x), ptr(a), ptr(rs), ptr(gb), ptr(bb),
                               float(eb), int(norm_b is not None), ptr(z), ptr(y), ptr(st_b), stream_ptr())
    return z, y, st_b


def linear_norm_joint_fwd(x, weight, bias, norm_a, a, norm_b, y_dtype):
    """u = x @ weight^T + bias (x's dtype), z = a + LN_A(u) (fp32), y = LN_B(z) | cast(z): the Linear of the positional encoding with its
    joint in the epilogue (ptv3m1:285, 318-323; bit-identical to spconv_fwd + add_norm_fwd with normA).  a fp32 or x's dtype.
    Returns (u, z, y, statA, statB)."""
    require_cuda(x, weight, bias, a)
    x, weight, a = x.contiguous(), weight.contiguous(), a.contiguous()
    c_out, c_in = weight.shape[0], weight.shape[-1]
    if x.dtype != weight.dtype or c_in != c_out or not linear_joint_supported(c_in, c_out, x.dtype) or a.dtype not in (torch.float32, x.dtype):
        raise PtcoreError("linear_norm_joint_fwd: unsupported shape / dtype")
    n, dev = int(a.shape[0]), x.device
    u = torch.empty((n, c_out), dtype=x.dtype, device=dev)
    z = torch.empty((n, c_out), dtype=torch.float32, device=dev)
    y = torch.empty((n, c_out), dtype=y_dtype, device=dev) if y_dtype is not None else None
    st_a = torch.empty((2, n), dtype=torch.float32, device=dev)
    st_b = torch.empty((2, n), dtype=torch.float32, device=dev) if (norm_b is not None and y is not None) else None
    ga, ba, ea = norm_a
    gb, bb, eb = norm_b if norm_b is not None else (None, None, 0.0)
    b = None if bias is None else bias.float().contiguous()
    lib().ptc_linear_norm_joint_fwd(ptr(x), x.shape[0], ptr(weight), ptr(b), n, c_in, c_out, dtype_code(x), ptr(ga), ptr(ba), float(ea), ptr(a),
                                    dtype_code(a), ptr(gb), ptr(bb), float(eb), int(norm_b is not None), ptr(u), ptr(z), ptr(y), ptr(st_a), ptr(st_b),
                                    stream_ptr())
    return u, z, y, st_a, st_b


def add_norm_bwd(dz_in, dy, z, u, row_scale, g_a, st_a, g_b, st_b, want_affine_a: bool, want_affine_b: bool,
                 da_dtype: torch.dtype = torch.float32):
    """-> (da (da_dtype: the dtype of the forward's `a`), du (u.dtype), dgA, dbA, dgB, dbB)"""
    require_cuda(dz_in, dy, z, u, row_scale)
    n, c = u.shape
    dev = u.device
    dz_in = None if dz_in is None else dz_in.to(torch.float32).contiguous()
    dy = None if dy is None else dy.contiguous()
    da = torch.empty((n, c), dtype=da_dtype, device=dev)
    du = torch.empty_like(u)
    mk = lambda want: torch.empty(c, dtype=torch.float32, device=dev) if want else None  # noqa: E731
    dga, dba, dgb, dbb = mk(want_affine_a), mk(want_affine_a), mk(want_affine_b), mk(want_affine_b)
    nbytes = lib().ptc_add_norm_bwd_workspace_bytes(n, c)
    ws = _ws(nbytes, dev)
    lib().ptc_add_norm_bwd(ptr(dz_in), ptr(dy), dtype_code(dy) if dy is not None else 0, ptr(z), ptr(u), dtype_code(u),
                           ptr(row_scale), n, c, ptr(g_a), ptr(st_a), int(st_a is not None), ptr(g_b), ptr(st_b),
                           int(st_b is not None), ptr(da), dtype_code(da), ptr(du), ptr(dga), ptr(dba), ptr(dgb), ptr(dbb), ptr(ws),
                           nbytes, stream_ptr())
    return da, du, dga, dba, dgb, dbb


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def attn_hd_supported(head_dim: int, max_seqlen: int) -> bool:
    """True when the window-attention kernels serve (head_dim, max_seqlen): head_dim 16 .. 64, max_seqlen bounded by LDS (ptcore.h, H)."""
    return bool(_ask("ptc_attn_varlen_hd_supported", int(head_dim), int(max_seqlen)))


def attn_varlen_fwd(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int, softmax_scale: float, dropout_p: float = 0.0, seed: int = 0):
    """qkv [T,3,H,D] bf16 -> (out [T,H,D] bf16, lse [H,T] fp32); D = 16 (attention.hip) or 17..64 (attention_hd.h).
    D = 16 also takes f16 qkv: the SAME bf16 arithmetic with the reference's qkv.to(bfloat16) / feat.to(qkv.dtype) casts
    (ptv3m1:209,215) done in the kernel's load / store paths -- out comes back f16, bit for bit what the two cast passes produce.
    D = 17..64 with f16 qkv: f16 operands (f16 MFMAs, P rounded to f16), LitePT's call site."""
    require_cuda(qkv, cu_seqlens)
    if qkv.dtype not in (torch.bfloat16, torch.float16) or qkv.dim() != 4 or qkv.shape[1] != 3:
        raise PtcoreError(f"qkv must be bf16 or f16 [T,3,H,D], got {qkv.dtype} {tuple(qkv.shape)}")
    qkv = qkv.contiguous()
    cu = cu_seqlens.to(torch.int32).contiguous()
    T, _, H, D = qkv.shape
    out = torch.empty((T, H, D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((H, T), dtype=torch.float32, device=qkv.device)
    if dropout_p > 0.0:       # attention dropout (csrc/attention_drop.h): head_dim 16; the mask is a function of `seed`, regenerated by the backward
        if D != ATTN_HEAD_DIM:
            raise PtcoreError(f"attention dropout is implemented for head_dim {ATTN_HEAD_DIM}")
        lib().ptc_attn_varlen_dropout_fwd(ptr(qkv), ptr(cu), cu.numel() - 1, T, H, int(max_seqlen), float(softmax_scale), dtype_code(qkv),
                                          float(dropout_p), int(seed), ptr(out), ptr(lse), stream_ptr())
    elif D == ATTN_HEAD_DIM:
        lib().ptc_attn_varlen_fwd(ptr(qkv), ptr(cu), cu.numel() - 1, T, H, int(max_seqlen), float(softmax_scale),
                                  dtype_code(qkv), ptr(out), ptr(lse), stream_ptr())
    else:
        lib().ptc_attn_varlen_hd_fwd(ptr(qkv), ptr(cu), cu.numel() - 1, T, H, D, int(max_seqlen), float(softmax_scale),
                                     dtype_code(qkv), ptr(out), ptr(lse), stream_ptr())
    return out, lse


def attn_varlen_bwd(qkv, out, dout, lse, cu_seqlens, max_seqlen: int, softmax_scale: float, dropout_p: float = 0.0, seed: int = 0) -> torch.Tensor:
    require_cuda(qkv, out, dout, lse, cu_seqlens)
    qkv = qkv.contiguous()
    out = out.contiguous()
    dout = dout.to(qkv.dtype).contiguous()       # (f16 qkv, D = 16: f16 out / dout / dqkv, the casts live in the kernels, see attn_varlen_fwd)
    cu = cu_seqlens.to(torch.int32).contiguous()
    T, _, H, D = qkv.shape
    dqkv = torch.empty_like(qkv)
    nbytes = lib().ptc_attn_varlen_bwd_workspace_bytes(T, H)
    ws = _ws(nbytes, qkv.device)
    if dropout_p > 0.0:
        lib().ptc_attn_varlen_dropout_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(cu), cu.numel() - 1, T, H, int(max_seqlen),
                                          float(softmax_scale), dtype_code(qkv), float(dropout_p), int(seed), ptr(dqkv), ptr(ws), nbytes,
                                          stream_ptr())
    elif D == ATTN_HEAD_DIM:
        lib().ptc_attn_varlen_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(cu), cu.numel() - 1, T, H,
                                  int(max_seqlen), float(softmax_scale), dtype_code(qkv), ptr(dqkv), ptr(ws), nbytes,
                                  stream_ptr())
    else:
        lib().ptc_attn_varlen_hd_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(cu), cu.numel() - 1, T, H, D,
                                     int(max_seqlen), float(softmax_scale), dtype_code(qkv), ptr(dqkv), ptr(ws), nbytes,
                                     stream_ptr())
    return dqkv


def attn_rope_supported(head_dim: int, max_seqlen: int) -> bool:
    """window attention with the 3-D rotary embedding fused into its prologue / epilogue (csrc/attention_hd.h, ROPE): head_dim 18"""
    return bool(lib().ptc_attn_varlen_hd_rope_supported(int(head_dim), int(max_seqlen)))


def attn_rope_fwd(qkv, xyz, inv_freq, cu_seqlens, max_seqlen: int, softmax_scale: float):
    """qkv [T,3,H,18] bf16 | f16, UN-rotated; xyz [T,3] fp32 positions of the (padded, serialized) rows; inv_freq [3] fp32
    -> (out [T,H,18], lse [H,T] fp32) of the attention over the rotated q / k."""
    require_cuda(qkv, xyz, inv_freq, cu_seqlens)
    if qkv.dtype not in (torch.bfloat16, torch.float16) or qkv.dim() != 4 or qkv.shape[1] != 3:
        raise PtcoreError(f"qkv must be bf16 or f16 [T,3,H,18], got {qkv.dtype} {tuple(qkv.shape)}")
    qkv, xyz, inv_freq = qkv.contiguous(), xyz.float().contiguous(), inv_freq.float().contiguous()
    T, _, H, D = qkv.shape
    if xyz.shape != (T, 3) or inv_freq.numel() * 6 != D:
        raise PtcoreError("attn_rope_fwd: xyz must be [T, 3] and inv_freq [head_dim / 6]")
    cu = cu_seqlens.to(torch.int32).contiguous()
    out = torch.empty((T, H, D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((H, T), dtype=torch.float32, device=qkv.device)
    lib().ptc_attn_varlen_hd_rope_fwd(ptr(qkv), ptr(cu), ptr(xyz), ptr(inv_freq), cu.numel() - 1, T, H, D, int(max_seqlen),
                                      float(softmax_scale), dtype_code(qkv), ptr(out), ptr(lse), stream_ptr())
    return out, lse


def attn_rope_bwd(qkv, out, dout, lse, xyz, inv_freq, cu_seqlens, max_seqlen: int, softmax_scale: float) -> torch.Tensor:
    """-> dqkv: gradient of the UN-rotated rows (the inverse rotation of dq / dk happens in the kernels' epilogue)"""
    require_cuda(qkv, out, dout, lse, xyz, inv_freq, cu_seqlens)
    qkv, out = qkv.contiguous(), out.contiguous()
    dout = dout.to(qkv.dtype).contiguous()
    xyz, inv_freq = xyz.float().contiguous(), inv_freq.float().contiguous()
    cu = cu_seqlens.to(torch.int32).contiguous()
    T, _, H, D = qkv.shape
    dqkv = torch.empty_like(qkv)
    nbytes = lib().ptc_attn_varlen_bwd_workspace_bytes(T, H)
    ws = _ws(nbytes, qkv.device)
    lib().ptc_attn_varlen_hd_rope_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(cu), ptr(xyz), ptr(inv_freq), cu.numel() - 1, T, H, D,
                                      int(max_seqlen), float(softmax_scale), dtype_code(qkv), ptr(dqkv), ptr(ws), nbytes, stream_ptr())
    return dqkv


def attn_rpe_supported(head_dim: int, max_seqlen: int, pos_bnd: int, dtype: torch.dtype = torch.bfloat16) -> bool:
    """RPE attention kernels: head_dim 16, window images + coordinates + table within the LDS budget of forward and backward"""
    return dtype in _DT and bool(_ask("ptc_attn_rpe_supported", int(head_dim), int(max_seqlen), int(pos_bnd), _DT[dtype]))


def attn_rpe_fwd(qkv, cu_seqlens, max_seqlen: int, softmax_scale: float, grid_coord, rpe_table, pos_bnd: int):
    """qkv [T,3,H,16] bf16 | f16 | fp32, grid_coord [T,3] int32 (same row order), rpe_table [3(2B+1),H] fp32 -> (out [T,H,16] like qkv,
    lse [H,T] fp32).  f16 tensors (the reference's fp16 AMP) ride around the same bf16 arithmetic: the casts sit in the kernels' load /
    store paths.  fp32 tensors (no autocast) run the fp32 kernels: fp32 operands, logits, softmax and accumulation."""
    require_cuda(qkv, cu_seqlens, grid_coord, rpe_table)
    if qkv.dtype not in (torch.bfloat16, torch.float16, torch.float32) or qkv.dim() != 4 or qkv.shape[1] != 3 or qkv.shape[3] != ATTN_HEAD_DIM:
        raise PtcoreError(f"qkv must be bf16 / f16 / fp32 [T,3,H,{ATTN_HEAD_DIM}], got {qkv.dtype} {tuple(qkv.shape)}")
    T, _, H, _ = qkv.shape
    if grid_coord.dtype != torch.int32 or tuple(grid_coord.shape) != (T, 3):
        raise PtcoreError(f"grid_coord must be int32 [{T},3], got {grid_coord.dtype} {tuple(grid_coord.shape)}")
    if rpe_table.dtype != torch.float32 or tuple(rpe_table.shape) != (3 * (2 * int(pos_bnd) + 1), H):
        raise PtcoreError(f"rpe_table must be fp32 [{3 * (2 * int(pos_bnd) + 1)},{H}], got {rpe_table.dtype} {tuple(rpe_table.shape)}")
    qkv, gc, tab = qkv.contiguous(), grid_coord.contiguous(), rpe_table.contiguous()
    cu = cu_seqlens.to(torch.int32).contiguous()
    out = torch.empty((T, H, 16), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((H, T), dtype=torch.float32, device=qkv.device)
    lib().ptc_attn_rpe_fwd(ptr(qkv), ptr(cu), ptr(gc), ptr(tab), int(pos_bnd), cu.numel() - 1, T, H, int(max_seqlen),
                           float(softmax_scale), dtype_code(qkv), ptr(out), ptr(lse), stream_ptr())
    return out, lse


def attn_rpe_bwd(qkv, out, dout, lse, cu_seqlens, max_seqlen: int, softmax_scale: float, grid_coord, rpe_table, pos_bnd: int):
    """-> (dqkv like qkv, d_rpe_table fp32 like rpe_table).  qkv / out / dout bf16 | f16 | fp32 (dout is cast to qkv's dtype); the
    fp32 table gradient is exact to 2^-44 per entry and bit-reproducible, NaN in a head whose sum of |dS| reaches 2^18 (ptcore.h)."""
    require_cuda(qkv, out, dout, lse, cu_seqlens, grid_coord, rpe_table)
    qkv, out = qkv.contiguous(), out.contiguous()
    dout = dout.to(qkv.dtype).contiguous()
    gc, tab = grid_coord.contiguous(), rpe_table.contiguous()
    cu = cu_seqlens.to(torch.int32).contiguous()
    T, _, H, _ = qkv.shape
    dqkv = torch.empty_like(qkv)
    dtab = torch.empty_like(tab)
    nbytes = lib().ptc_attn_rpe_bwd_workspace_bytes(T, H, int(pos_bnd))
    ws = _ws(nbytes, qkv.device)
    lib().ptc_attn_rpe_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(cu), ptr(gc), ptr(tab), int(pos_bnd), cu.numel() - 1,
                           T, H, int(max_seqlen), float(softmax_scale), dtype_code(qkv), ptr(dqkv), ptr(dtab), ptr(ws), nbytes,
                           stream_ptr())
    return dqkv, dtab


# ------------------------------------------------------------------------------------------------
# ends of the step: coordinate maxima, cross-entropy
# ------------------------------------------------------------------------------------------------
def coord_max(grid_coord: torch.Tensor) -> torch.Tensor:
    """max over points of grid_coord per axis -> int64 [3] on the device (structure.py:74,136-138)."""
    require_cuda(grid_coord)
    if grid_coord.dtype not in (torch.int64, torch.int32) or grid_coord.dim() != 2 or grid_coord.shape[1] != 3:
        raise PtcoreError("grid_coord must be int32/int64 [N,3]")
    gc = grid_coord.contiguous()
    out = torch.empty(3, dtype=torch.int64, device=gc.device)
    lib().ptc_coord_max(ptr(gc), int(gc.dtype == torch.int64), gc.shape[0], ptr(out), stream_ptr())
    return out


def _rows_view(t: torch.Tensor):
    """[N, C] tensor whose rows are contiguous (any row stride) -> (tensor, row_stride)"""
    if t.dim() != 2:
        raise PtcoreError("expected [N, C]")
    if t.shape[0] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def cross_entropy_fwd(logits: torch.Tensor, target: torch.Tensor, ignore_index: int):
    """-> (loss_sum [] fp32, count [] fp32, lse [N] fp32); loss = loss_sum / count (CrossEntropyLoss, mean)."""
    require_cuda(logits, target)
    if target.dtype != torch.int64:
        raise PtcoreError("target must be int64")
    lg, rs = _rows_view(logits)
    n, c = lg.shape
    nb = lib().ptc_cross_entropy_partials(n)
    lse = torch.empty(n, dtype=torch.float32, device=lg.device)
    partial = torch.empty((nb, 2), dtype=torch.float32, device=lg.device)
    lib().ptc_cross_entropy_fwd(ptr(lg), rs, ptr(target.contiguous()), n, c, dtype_code(lg), int(ignore_index), ptr(lse),
                                ptr(partial), stream_ptr())
    tot = partial.sum(0)   # fixed-order tree reduction of <= N/256 partials: deterministic
    return tot[0], tot[1], lse


def cross_entropy_bwd(logits: torch.Tensor, target: torch.Tensor, lse: torch.Tensor, scale: torch.Tensor, ignore_index: int):
    """dlogits [N, C] (logits' dtype) = scale * (softmax - onehot) on counted rows; `scale` device scalar fp32."""
    require_cuda(logits, target, lse, scale)
    lg, rs = _rows_view(logits)
    n, c = lg.shape
    out = torch.empty((n, c), dtype=lg.dtype, device=lg.device)
    lib().ptc_cross_entropy_bwd(ptr(lg), rs, ptr(target.contiguous()), ptr(lse), ptr(scale.reshape(1).float().contiguous()),
                                n, c, dtype_code(lg), int(ignore_index), ptr(out), c, stream_ptr())
    return out


CRITERIA_ROWS_MAX_C = _K["PTC_CRITERIA_ROWS_MAX_C"]     # the register-row path (csrc/loss_rows.h) serves every term
CRITERIA_CE_MAX_C = _K["PTC_CRITERIA_CE_MAX_C"]         # wider rows: the cross-entropy term alone, element-wise
CRITERIA_CE, CRITERIA_FOCAL, CRITERIA_DICE = (_K[k] for k in ("PTC_CRITERIA_CE", "PTC_CRITERIA_FOCAL", "PTC_CRITERIA_DICE"))


class CriteriaSpec:
    """The terms of one fused criteria call (csrc/criteria.hip), as the kernels take them: `flags` (CRITERIA_* bits) and per term its
    loss_weight and settings; ce_weight / focal_alpha_vec are fp32 [C] tensors on the logits' device or None."""

    __slots__ = ("flags", "ignore_index", "ce_weight", "ce_eps", "ce_sum", "ce_lw", "focal_alpha", "focal_alpha_vec", "focal_gamma",
                 "focal_lw", "dice_smooth", "dice_exp", "dice_lw")

    def __init__(self, ignore_index: int = -1):
        self.flags, self.ignore_index = 0, int(ignore_index)
        self.ce_weight, self.ce_eps, self.ce_sum, self.ce_lw = None, 0.0, False, 1.0
        self.focal_alpha, self.focal_alpha_vec, self.focal_gamma, self.focal_lw = 0.5, None, 2.0, 1.0
        self.dice_smooth, self.dice_exp, self.dice_lw = 1.0, 2, 1.0


def _criteria_check(spec: CriteriaSpec, lg: torch.Tensor):
    c = lg.shape[1]      # (the class limits CRITERIA_ROWS_MAX_C / CRITERIA_CE_MAX_C are the library's to refuse)
    for name, vec in (("weight", spec.ce_weight), ("alpha", spec.focal_alpha_vec)):
        if vec is not None and (vec.dtype != torch.float32 or vec.numel() != c or vec.device != lg.device or not vec.is_contiguous()):
            raise PtcoreError(f"criteria kernels: {name} must be a contiguous fp32 [{c}] tensor on the logits' device")


def criteria_rows_fwd(logits: torch.Tensor, target: torch.Tensor, spec: CriteriaSpec):
    """-> (out [4] fp32 = total, ce, focal, dice -- each term times its loss_weight --, lsum [N] fp32 = log sum_j exp(x_j - max x),
    coef [4 + 2C] fp32 for criteria_rows_bwd).  One kernel over the rows, the per-workgroup partial rows summed in double in a fixed order, one finish
    launch; no host read."""
    require_cuda(logits, target)
    if target.dtype != torch.int64:
        raise PtcoreError("target must be int64")
    lg, rs = _rows_view(logits)
    n, c = lg.shape
    _criteria_check(spec, lg)
    nb, pw = lib().ptc_criteria_partials(n), lib().ptc_criteria_partial_width(c, spec.flags)
    lse = torch.empty(n, dtype=torch.float32, device=lg.device)
    partial = torch.empty((nb, pw), dtype=torch.float32, device=lg.device)
    lib().ptc_criteria_fwd(ptr(lg), rs, ptr(target.contiguous()), n, c, dtype_code(lg), spec.ignore_index, spec.flags,
                           ptr(spec.ce_weight), float(spec.ce_eps), ptr(spec.focal_alpha_vec), float(spec.focal_alpha),
                           float(spec.focal_gamma), int(spec.dice_exp), ptr(lse), ptr(partial), stream_ptr())
    sums = partial.sum(0, dtype=torch.float64)       # fixed-order reduction of <= N/256 partial rows: deterministic
    out = torch.empty(4, dtype=torch.float32, device=lg.device)
    coef = torch.empty(4 + 2 * c, dtype=torch.float32, device=lg.device)
    lib().ptc_criteria_finish(ptr(sums), c, spec.flags, spec.ignore_index, ptr(spec.ce_weight), int(bool(spec.ce_sum)),
                              float(spec.ce_lw), float(spec.focal_lw), float(spec.dice_lw), float(spec.dice_smooth),
                              int(spec.dice_exp), ptr(out), ptr(coef), stream_ptr())
    return out, lse, coef


def criteria_rows_bwd(logits: torch.Tensor, target: torch.Tensor, lse: torch.Tensor, coef: torch.Tensor, grad: torch.Tensor,
                      spec: CriteriaSpec) -> torch.Tensor:
    """dlogits [N, C] (logits' dtype, dense) = grad * d total / d logits; `grad` device scalar."""
    require_cuda(logits, target, lse, coef, grad)
    lg, rs = _rows_view(logits)
    n, c = lg.shape
    _criteria_check(spec, lg)
    out = torch.empty((n, c), dtype=lg.dtype, device=lg.device)
    lib().ptc_criteria_bwd(ptr(lg), rs, ptr(target.contiguous()), ptr(lse), ptr(coef), ptr(grad.reshape(1).float().contiguous()),
                           n, c, dtype_code(lg), spec.ignore_index, spec.flags, ptr(spec.ce_weight), float(spec.ce_eps),
                           ptr(spec.focal_alpha_vec), float(spec.focal_alpha), float(spec.focal_gamma), int(spec.dice_exp),
                           ptr(out), stream_ptr())
    return out


LOVASZ_DENSE_MAX_C = _K["PTC_LOVASZ_DENSE_MAX_C"]       # the dense [C, N] path (csrc/lovasz.hip LV_MAX_C)
LOVASZ_MAX_C = _K["PTC_LOVASZ_MAX_C"]                   # the row-compacted path (LW_MAX_C)


class LovaszPresent:
    """What ptc_lovasz_present leaves on the device for one (target, num_classes, ignore_index): class_count / row_of / class_of [C]
    and n_present [1] (int32), the copy of n_present on its way into pinned host memory, and the identity of `target` (data pointer,
    shape, version counter) the handle is valid for."""

    __slots__ = ("class_count", "row_of", "class_of", "n_present", "num_classes", "ignore_index", "_host", "_event", "_target", "_ident")

    def __init__(self, target, num_classes, ignore_index, class_count, row_of, class_of, n_present, host, event):
        self.class_count, self.row_of, self.class_of, self.n_present = class_count, row_of, class_of, n_present
        self.num_classes, self.ignore_index = int(num_classes), int(ignore_index)
        self._host, self._event = host, event
        self._target = target                      # kept alive: its storage cannot be handed to another tensor meanwhile
        self._ident = _target_ident(target)

    def rows(self) -> int:
        """P on the host; waits for the copy only if it has not landed yet"""
        if self._event is not None:
            self._event.synchronize()
            self._event = None
        return int(self._host[0])

    def matches(self, target, num_classes, ignore_index) -> bool:
        return (self._ident == _target_ident(target) and self.num_classes == int(num_classes) and self.ignore_index == int(ignore_index))


def _target_ident(target):
    return (target.data_ptr(), tuple(target.shape), tuple(target.stride()), target._version, target.device)


def lovasz_present(target: torch.Tensor, num_classes: int, ignore_index: int) -> LovaszPresent:
    """The classes with at least one counted label, ranked, for lovasz_softmax(..., present=handle): everything stays on the device
    and on the current stream; P travels to pinned host memory behind an event, so a caller that asks early (the segmentor: before
    the backbone) finds it there when the loss needs it."""
    require_cuda(target)
    if target.dtype != torch.int64 or target.dim() != 1:
        raise PtcoreError("target must be int64 [N]")
    c = int(num_classes)
    tg = target.contiguous()
    buf = torch.empty(3 * c + 1, dtype=torch.int32, device=tg.device)
    count, row_of, class_of, n_present = buf[:c], buf[c:2 * c], buf[2 * c:3 * c], buf[3 * c:]
    lib().ptc_lovasz_present(ptr(tg), tg.shape[0], c, int(ignore_index), ptr(count), ptr(row_of), ptr(class_of), ptr(n_present),
                             stream_ptr())
    if tg.is_cuda:
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(n_present, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
    else:
        host, event = n_present, None
    return LovaszPresent(target, c, ignore_index, count, row_of, class_of, n_present, host, event)


def lovasz_softmax(logits: torch.Tensor, target: torch.Tensor, ignore_index: int, present: Optional[LovaszPresent] = None):
    """Lovasz-Softmax (multiclass, classes present, whole batch: pointcept/models/losses/lovasz.py:118-146) ->
    (loss [] fp32, dlogits [N, C] fp32).  C <= 64 without a handle: one segmented radix sort of the dense [C, N] error matrix.
    65 <= C <= 1024, or any C with `present` (lovasz_present of the same target): the sort runs over the P classes present only
    ([P, N], ~56 B x P x N of workspace); without a handle one is made here, and reading P is this path's one host synchronisation.
    A handle of another target (or of this one edited in place since), class count or ignore_index is refused before any launch."""
    require_cuda(logits, target)
    if target.dtype != torch.int64:
        raise PtcoreError("target must be int64")
    lg, rs = _rows_view(logits)
    n, c = lg.shape
    if present is None and c > LOVASZ_DENSE_MAX_C:       # (past LOVASZ_MAX_C the library refuses)
        present = lovasz_present(target, c, ignore_index)
    if present is not None:
        return _lovasz_softmax_rows(lg, rs, target, ignore_index, present)
    nbytes = lib().ptc_lovasz_softmax_workspace_bytes(n, c)
    if nbytes == 0:
        raise PtcoreError(f"lovasz_softmax: unsupported shape [{n}, {c}]")
    ws = _ws(nbytes, lg.device)
    loss = torch.empty((), dtype=torch.float32, device=lg.device)
    dlogits = torch.empty((n, c), dtype=torch.float32, device=lg.device)
    lib().ptc_lovasz_softmax(ptr(lg), rs, ptr(target.contiguous()), n, c, dtype_code(lg), int(ignore_index), ptr(loss),
                             ptr(dlogits), ptr(ws), nbytes, stream_ptr())
    return loss, dlogits


def _lovasz_softmax_rows(lg, rs, target, ignore_index, present):
    n, c = lg.shape
    if not isinstance(present, LovaszPresent):
        raise PtcoreError("lovasz_softmax: `present` must come from lovasz_present")
    if target.dim() != 1 or target.shape[0] != n:
        raise PtcoreError("lovasz_softmax: target must be [N]")
    if not present.matches(target, c, ignore_index):
        raise PtcoreError("lovasz_softmax: `present` was made from another target (or the target was edited in place since), "
                          "another number of classes or another ignore_index")
    rows = present.rows()
    if not 0 <= rows <= c:
        raise PtcoreError(f"lovasz_softmax: {rows} present classes of {c}")
    nbytes = lib().ptc_lovasz_softmax_rows_workspace_bytes(n, c, rows)
    ws = _ws(nbytes, lg.device)
    loss = torch.empty((), dtype=torch.float32, device=lg.device)
    dlogits = torch.empty((n, c), dtype=torch.float32, device=lg.device)
    lib().ptc_lovasz_softmax_rows(ptr(lg), rs, ptr(target.contiguous()), n, c, dtype_code(lg), int(ignore_index), ptr(present.class_count),
                                  ptr(present.row_of), ptr(present.class_of), ptr(present.n_present), rows, ptr(loss), ptr(dlogits),
                                  ptr(ws), nbytes, stream_ptr())
    return loss, dlogits


# ------------------------------------------------------------------------------------------------
# BatchNorm1d + activation
# ------------------------------------------------------------------------------------------------
ACT_CODES = {k[len("PTC_ACT_"):].lower(): v for k, v in _lib.HEADER.enums["ptc_act"].items()}       # "none": 0, ...


def batch_norm_supported(c: int, dtype: torch.dtype) -> bool:
    return dtype in _DT and bool(lib().ptc_batch_norm_supported(int(c), _DT[dtype]))


def batch_norm_act_fwd(x, gamma, beta, running_mean, running_var, training: bool, momentum: float, eps: float, act: str,
                       out_dtype: Optional[torch.dtype] = None, res: Optional[torch.Tensor] = None):
    """-> (y [N,C] out_dtype, save_mean [C] f32, save_rstd [C] f32); running statistics updated in place.  res [N,C] (x's dtype):
    y = act(BN(x) + res), the tail of a residual block in the same apply pass (ptc_batch_norm_add_act_fwd)."""
    require_cuda(x, gamma, beta, running_mean, running_var, res)
    x = x.contiguous()
    if res is not None:
        if res.shape != x.shape or res.dtype != x.dtype:
            raise PtcoreError("batch_norm_act_fwd: the residual must have x's shape and dtype")
        res = res.contiguous()
    n, c = x.shape
    out_dtype = out_dtype or x.dtype
    y = torch.empty((n, c), dtype=out_dtype, device=x.device)
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    rstd = torch.empty(c, dtype=torch.float32, device=x.device)
    nbytes = lib().ptc_batch_norm_workspace_bytes(n, c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    g = None if gamma is None else gamma.float().contiguous()
    b = None if beta is None else beta.float().contiguous()
    for t in (running_mean, running_var):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise PtcoreError("running statistics must be contiguous fp32")
    if res is not None:
        lib().ptc_batch_norm_add_act_fwd(ptr(x), ptr(res), n, c, dtype_code(x), ptr(g), ptr(b), float(eps), float(momentum),
                                         int(bool(training)), ptr(running_mean), ptr(running_var), ACT_CODES[act], ptr(y),
                                         dtype_code(y), ptr(mean), ptr(rstd), ptr(ws), nbytes, stream_ptr())
        return y, mean, rstd
    lib().ptc_batch_norm_act_fwd(ptr(x), n, c, dtype_code(x), ptr(g), ptr(b), float(eps), float(momentum), int(bool(training)),
                                 ptr(running_mean), ptr(running_var), ACT_CODES[act], ptr(y), dtype_code(y), ptr(mean),
                                 ptr(rstd), ptr(ws), nbytes, stream_ptr())
    return y, mean, rstd


def batch_norm_act_bwd(dy, x, gamma, beta, mean, rstd, training: bool, act: str, want_affine: bool = True, res: Optional[torch.Tensor] = None):
    """-> (dx [N,C] x.dtype, dgamma [C] f32 | None, dbeta [C] f32 | None); with res (the forward's residual): a fourth result dres [N,C]"""
    require_cuda(dy, x, mean, rstd, res)
    dy, x = dy.contiguous(), x.contiguous()
    n, c = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(c, dtype=torch.float32, device=x.device) if want_affine else None
    db = torch.empty(c, dtype=torch.float32, device=x.device) if want_affine else None
    nbytes = lib().ptc_batch_norm_workspace_bytes(n, c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    g = None if gamma is None else gamma.float().contiguous()
    b = None if beta is None else beta.float().contiguous()
    if res is not None:
        res = res.contiguous()
        dres = torch.empty_like(x)
        lib().ptc_batch_norm_add_act_bwd(ptr(dy), dtype_code(dy), ptr(x), ptr(res), dtype_code(x), ptr(g), ptr(b), ptr(mean), ptr(rstd), n, c,
                                         int(bool(training)), ACT_CODES[act], ptr(dx), ptr(dres), ptr(dg), ptr(db), ptr(ws), nbytes,
                                         stream_ptr())
        return dx, dg, db, dres
    lib().ptc_batch_norm_act_bwd(ptr(dy), dtype_code(dy), ptr(x), dtype_code(x), ptr(g), ptr(b), ptr(mean), ptr(rstd), n, c,
                                 int(bool(training)), ACT_CODES[act], ptr(dx), ptr(dg), ptr(db), ptr(ws), nbytes, stream_ptr())
    return dx, dg, db


def column_sum(x: torch.Tensor) -> torch.Tensor:
    """x [N, C] (f32 / bf16 / f16) -> fp32 [C] = x.float().sum(0) in one read of x (bias gradients)."""
    require_cuda(x)
    if x.dim() != 2:
        raise PtcoreError("column_sum expects [N, C]")
    if not batch_norm_supported(x.shape[1], x.dtype):
        return x.float().sum(0)          # odd channel counts: ATen on the GPU
    x = x.contiguous()
    n, c = x.shape
    out = torch.empty(c, dtype=torch.float32, device=x.device)
    nbytes = lib().ptc_batch_norm_workspace_bytes(n, c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    lib().ptc_column_sum(ptr(x), n, c, dtype_code(x), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


def linear_supported_ex(c_in: int, c_out: int, dtype: torch.dtype) -> bool:
    return dtype in _DT and bool(lib().ptc_linear_supported_ex(int(c_in), int(c_out), _DT[dtype]))


def linear_gelu_fwd(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]):
    """(h, a) = (x W^T + b, GELU(h)) in one kernel; x [N, C_in], weight [C_out, C_in] (both bf16 / f16)."""
    require_cuda(x, weight, bias)
    x, weight = x.contiguous(), weight.contiguous()
    n, c_in = x.shape
    c_out = weight.shape[0]
    h = torch.empty((n, c_out), dtype=x.dtype, device=x.device)
    a = torch.empty((n, c_out), dtype=x.dtype, device=x.device)
    b = None if bias is None else bias.to(torch.float32).contiguous()
    lib().ptc_linear_fwd_ex(ptr(x), n, ptr(weight), ptr(b), c_in, c_out, dtype_code(x), 1, 0, ptr(h), ptr(a), stream_ptr())
    return h, a


def linear_gelu_bwd_input(g: torch.Tensor, weight_t: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """dh = (g W) * GELU'(h) in one kernel; g [N, C_out2], weight_t [hidden, C_out2] (= W2^T), h [N, hidden]."""
    require_cuda(g, weight_t, h)
    g, weight_t, h = g.contiguous(), weight_t.contiguous(), h.contiguous()
    n, c_in = g.shape
    c_out = weight_t.shape[0]
    out = torch.empty((n, c_out), dtype=g.dtype, device=g.device)
    lib().ptc_linear_fwd_ex(ptr(g), n, ptr(weight_t), 0, c_in, c_out, dtype_code(g), 2, ptr(h), ptr(out), 0, stream_ptr())
    return out


def mlp_supported(c: int, dtype: torch.dtype) -> bool:
    """the one-kernel MLP (csrc/mlp.hip): C = 32 | 64 (hidden 4 C), bf16 / f16"""
    return dtype in _DT and bool(lib().ptc_mlp_supported(int(c), _DT[dtype]))


def block_mlp_fused(c: int, dtype: torch.dtype) -> bool:
    """mlp_supported and not PTC_BLK_MLP_FUSED=0, which the library alone reads: the block executor's answer, for the Python path too"""
    return dtype in _DT and bool(_ask("ptc_ptv3_block_mlp_fused", int(c), _DT[dtype]))


def mlp_fwd(x, w1, b1, w2, b2, a=None, row_scale=None, want_y=True):
    """m = GELU(x W1^T + b1) W2^T + b2 in one kernel.  a is None: -> m [N, C] (x's dtype).  a [N, C] fp32 (the residual stream):
    -> (z = a + row_scale * m fp32, y = cast(z) or None)."""
    require_cuda(x, w1, b1, w2, b2, a, row_scale)
    x, w1, w2 = x.contiguous(), w1.contiguous(), w2.contiguous()
    n, c = x.shape
    if tuple(w1.shape) != (4 * c, c) or tuple(w2.shape) != (c, 4 * c) or w1.dtype != x.dtype or w2.dtype != x.dtype:
        raise PtcoreError(f"mlp_fwd: x {tuple(x.shape)} {x.dtype}, w1 {tuple(w1.shape)} {w1.dtype}, w2 {tuple(w2.shape)} {w2.dtype}")
    b1 = None if b1 is None else b1.to(torch.float32).contiguous()
    b2 = None if b2 is None else b2.to(torch.float32).contiguous()
    if a is None:
        y = torch.empty((n, c), dtype=x.dtype, device=x.device)
        lib().ptc_mlp_fwd(ptr(x), n, c, dtype_code(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), 0, 0, 0, ptr(y), stream_ptr())
        return y
    if a.dtype != torch.float32 or tuple(a.shape) != (n, c):
        raise PtcoreError("mlp_fwd: the residual stream must be fp32 [N, C]")
    a = a.contiguous()
    rs = None if row_scale is None else row_scale.to(torch.float32).contiguous()
    z = torch.empty((n, c), dtype=torch.float32, device=x.device)
    y = torch.empty((n, c), dtype=x.dtype, device=x.device) if want_y else None
    lib().ptc_mlp_fwd(ptr(x), n, c, dtype_code(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(a), ptr(rs), ptr(z), ptr(y), stream_ptr())
    return z, y


def mlp_bwd(dm, x, w1, b1, w2t, want_b1=True, want_b2=True):
    """-> (dx [N, C] like x, dw1 [4C, C], db1 [4C] | None, dw2 [C, 4C], db2 [C] | None), fp32 parameter gradients; w2t = W2^T [4C, C]."""
    require_cuda(dm, x, w1, b1, w2t)
    dm, x, w1, w2t = dm.contiguous(), x.contiguous(), w1.contiguous(), w2t.contiguous()
    n, c = x.shape
    hid = 4 * c
    if dm.shape != x.shape or dm.dtype != x.dtype or tuple(w1.shape) != (hid, c) or tuple(w2t.shape) != (hid, c) or w1.dtype != x.dtype or w2t.dtype != x.dtype:
        raise PtcoreError(f"mlp_bwd: dm {tuple(dm.shape)} {dm.dtype}, x {tuple(x.shape)} {x.dtype}, w1 {tuple(w1.shape)}, w2t {tuple(w2t.shape)}")
    b1 = None if b1 is None else b1.to(torch.float32).contiguous()
    dx = torch.empty_like(x)
    dw1 = torch.empty((hid, c), dtype=torch.float32, device=x.device)
    dw2 = torch.empty((c, hid), dtype=torch.float32, device=x.device)
    db1 = torch.empty((hid,), dtype=torch.float32, device=x.device) if want_b1 else None
    db2 = torch.empty((c,), dtype=torch.float32, device=x.device) if want_b2 else None
    nbytes = lib().ptc_mlp_bwd_workspace_bytes(n, c)
    ws = _ws(nbytes, x.device)
    lib().ptc_mlp_bwd(ptr(dm), ptr(x), n, c, dtype_code(x), ptr(w1), ptr(b1), ptr(w2t), ptr(dx), ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), ptr(ws), nbytes,
                      stream_ptr())
    return dx, dw1, db1, dw2, db2


def weight_layouts(desc: torch.Tensor, prefix: torch.Tensor, n: int, total: int) -> None:
    """functional._CastCache: rewrite every backward-pass weight layout described by desc [n,6] / prefix [n+1] (device int64)."""
    require_cuda(desc, prefix)
    lib().ptc_weight_layouts(ptr(desc), ptr(prefix), int(n), int(total), stream_ptr())


def cast_many(desc: torch.Tensor, prefix: torch.Tensor, n: int, total_units: int, dst_dtype: torch.dtype) -> None:
    """functional._CastCache: refresh the 16-bit shadows described by desc [n,3] / prefix [n+1] (device int64) from their fp32 weights."""
    require_cuda(desc, prefix)
    lib().ptc_cast_many(ptr(desc), ptr(prefix), int(n), int(total_units), _DT[dst_dtype], stream_ptr())


# ------------------------------------------------------------------------------------------------
# libs/pointops2: pair-list attention operators (csrc/pointops2.hip), fp32
# ------------------------------------------------------------------------------------------------
def _p2_check(name, t, shape=None, dtype=torch.float32):
    if t is None:
        return
    if t.dtype != dtype or not t.is_contiguous():
        raise PtcoreError(f"{name}: expected a contiguous {dtype} tensor, got {t.dtype} (contiguous={t.is_contiguous()})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise PtcoreError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def pair_dot_fwd(q, k, i0, i1, table_q, table_k, rel_idx, with_qk: bool) -> torch.Tensor:
    """out[m,h] = [with_qk] q[i0[m],h].k[i1[m],h] + [table_q] q[i0[m],h].Tq(m,h) + [table_k] k[i1[m],h].Tk(m,h)"""
    require_cuda(q, k, i0, i1, table_q, table_k, rel_idx)
    _, H, d = q.shape
    M = i0.numel()
    _p2_check("q", q)
    _p2_check("k", k, (k.shape[0], H, d) if k is not None else None)
    _p2_check("i0", i0, (M,), torch.int32)
    _p2_check("i1", i1, (M,), torch.int32)
    _p2_check("rel_idx", rel_idx, (M, 3), torch.int32)
    for nm, t in (("table_q", table_q), ("table_k", table_k)):
        _p2_check(nm, t, (t.shape[0], H, d, 3) if t is not None else None)
    out = torch.empty((M, H), dtype=torch.float32, device=q.device)
    lib().ptc_pair_dot_fwd(ptr(q), ptr(k), ptr(i0), ptr(i1), ptr(table_q), ptr(table_k), ptr(rel_idx), int(bool(with_qk)), M, H, d,
                           ptr(out), stream_ptr())
    return out


def pair_dot_bwd(g, q, k, i0, offsets, i1, table_q, table_k, rel_idx, with_qk: bool, want_q=True, want_k=True, want_tq=True,
                 want_tk=True):
    require_cuda(g, q, k, i0, offsets, i1, table_q, table_k, rel_idx)
    Nq, H, d = q.shape
    M = i0.numel()
    _p2_check("grad_out", g, (M, H))
    if offsets is not None and offsets.numel() != Nq + 1:
        raise PtcoreError(f"offsets must have {Nq + 1} entries (one segment per query row), got {offsets.numel()}")
    Nk = k.shape[0] if k is not None else 0
    L = table_q.shape[0] if table_q is not None else (table_k.shape[0] if table_k is not None else 0)
    dq = torch.empty_like(q) if want_q else None
    dk = torch.empty_like(k) if (want_k and k is not None) else None
    dtq = torch.empty_like(table_q) if (want_tq and table_q is not None) else None
    dtk = torch.empty_like(table_k) if (want_tk and table_k is not None) else None
    lib().ptc_pair_dot_bwd(ptr(g), ptr(q), ptr(k), ptr(i0), ptr(offsets), ptr(i1), ptr(table_q), ptr(table_k), ptr(rel_idx),
                           int(bool(with_qk)), M, Nq, Nk, L, H, d, ptr(dq), ptr(dk), ptr(dtq), ptr(dtk), stream_ptr())
    return dq, dk, dtq, dtk


def pair_aggregate_fwd(attn, v, i0, offsets, i1, table_v, rel_idx, n_q: int) -> torch.Tensor:
    """out[n,h,c] = sum_{m: i0[m] = n} attn[m,h] (v[i1[m],h,c] + [table_v] Tv(m,h,c)), out [n_q, H, d]"""
    require_cuda(attn, v, i0, offsets, i1, table_v, rel_idx)
    _, H, d = v.shape
    M = i1.numel()
    _p2_check("attn", attn, (M, H))
    _p2_check("v", v)
    _p2_check("i0", i0, (M,), torch.int32)
    _p2_check("i1", i1, (M,), torch.int32)
    _p2_check("rel_idx", rel_idx, (M, 3), torch.int32)
    _p2_check("table", table_v, (table_v.shape[0], H, d, 3) if table_v is not None else None)
    if offsets is not None and offsets.numel() != int(n_q) + 1:
        raise PtcoreError(f"offsets must have {int(n_q) + 1} entries, got {offsets.numel()}")
    out = torch.empty((int(n_q), H, d), dtype=torch.float32, device=v.device)
    lib().ptc_pair_aggregate_fwd(ptr(attn), ptr(v), ptr(i0), ptr(offsets), ptr(i1), ptr(table_v), ptr(rel_idx), M, int(n_q), H, d,
                                 ptr(out), stream_ptr())
    return out


def pair_aggregate_bwd(g, attn, v, i0, i1, table_v, rel_idx, want_attn=True, want_v=True, want_tv=True):
    require_cuda(g, attn, v, i0, i1, table_v, rel_idx)
    Nv, H, d = v.shape
    M = i1.numel()
    _p2_check("grad_out", g, (g.shape[0], H, d))
    L = table_v.shape[0] if table_v is not None else 0
    da = torch.empty_like(attn) if want_attn else None
    dv = torch.empty_like(v) if want_v else None
    dtv = torch.empty_like(table_v) if (want_tv and table_v is not None) else None
    lib().ptc_pair_aggregate_bwd(ptr(g), ptr(attn), ptr(v), ptr(i0), ptr(i1), ptr(table_v), ptr(rel_idx), M, Nv, L, H, d, ptr(da),
                                 ptr(dv), ptr(dtv), stream_ptr())
    return da, dv, dtv



# ------------------------------------------------------------------------------------------------
# OA-CNNs adaptive aggregation (csrc/cluster_agg.hip)
# ------------------------------------------------------------------------------------------------
class GridClusters:
    """The grid clusters of every level of one DonwBlock (oacnns_v1m1_base.py:160-164): per level the inverse `cluster` [N] int64
    (torch.unique's numbering), `order` [N] int64 (rows in cluster order), the CSR `indptr` [n_cluster + 1] and `n_cluster` (host)."""

    def __init__(self, order, cluster, indptr, n_cluster):
        self.order, self.cluster, self.indptr, self.n_cluster = order, cluster, indptr, n_cluster

    @property
    def levels(self) -> int:
        return len(self.n_cluster)

    def _arrays(self):
        L = self.levels
        return ((ctypes.c_void_p * L)(*[ptr(t) for t in self.order]), (ctypes.c_void_p * L)(*[ptr(t) for t in self.indptr]),
                (ctypes.c_void_p * L)(*[ptr(t) for t in self.cluster]), (ctypes.c_int64 * L)(*self.n_cluster))


def grid_clusters(indices: torch.Tensor, sizes: Sequence[int], spatial_shape: Sequence[int], batch_size: int) -> GridClusters:
    """voxel_grid(indices[:, 1:].float(), size, indices[:, 0]) + torch.unique(return_inverse=True) for every size at once: one key
    pass, one sort of L rows, one count per level and ONE host read (the L cluster counts) for the whole block."""
    require_cuda(indices)
    if indices.dtype != torch.int32 or indices.dim() != 2 or indices.shape[1] != 4:
        raise PtcoreError("grid_clusters: indices must be int32 [N, 4] (batch, x, y, z)")
    if any(int(s) != s or int(s) < 1 for s in sizes):
        raise PtcoreError(f"grid_clusters: cell sizes must be positive integers, got {list(sizes)}")
    ind = indices.contiguous()
    n, L = ind.shape[0], len(sizes)
    dev = ind.device
    order = torch.empty((L, n), dtype=torch.int64, device=dev)
    cluster = torch.empty((L, n), dtype=torch.int64, device=dev)
    ncl = torch.empty(L, dtype=torch.int64, device=dev)
    nbytes = lib().ptc_grid_cluster_workspace_bytes(n, L)
    ws = _ws(nbytes, dev)
    sz = (ctypes.c_int * L)(*[int(s) for s in sizes])
    shp = (ctypes.c_int * 3)(*[int(s) for s in spatial_shape])
    lib().ptc_grid_cluster_count(ptr(ind), n, ctypes.cast(sz, ctypes.c_void_p), L, ctypes.cast(shp, ctypes.c_void_p), int(batch_size),
                                 ptr(order), ptr(cluster), ptr(ncl), ptr(ws), nbytes, stream_ptr())
    n_cluster = [int(v) for v in ncl.tolist()]
    indptr = []
    for l in range(L):
        ip = torch.empty(n_cluster[l] + 1, dtype=torch.int64, device=dev)
        head = torch.empty(n_cluster[l], dtype=torch.int64, device=dev)
        lib().ptc_pool_maps_fill(ptr(order[l]), ptr(cluster[l]), n, n_cluster[l], ptr(ip), ptr(head), stream_ptr())
        indptr.append(ip)
    return GridClusters(list(order.unbind(0)), list(cluster.unbind(0)), indptr, n_cluster)


def _agg_rows(ts, n: int, c: int, dtype, what: str):
    for t in ts:
        if t.dtype != dtype or t.shape != (n, c) or not t.is_contiguous():
            raise PtcoreError(f"{what}: every level tensor must be contiguous [{n}, {c}] {dtype}, got {tuple(t.shape)} {t.dtype}")


def cluster_center(xs: Sequence[torch.Tensor], gc: GridClusters) -> list:
    """y_l = x_l - scatter_mean(x_l, cluster_l)[cluster_l] for every level in one launch (oacnns_v1m1_base.py:92)."""
    require_cuda(*xs)
    L = gc.levels
    if len(xs) != L:
        raise PtcoreError(f"cluster_center: {len(xs)} tensors for {L} levels")
    xs = [x.contiguous() for x in xs]
    n, c = xs[0].shape
    _agg_rows(xs, n, c, xs[0].dtype, "cluster_center")
    ys = [torch.empty_like(x) for x in xs]
    perm, ip, _, ncl = gc._arrays()
    xa = (ctypes.c_void_p * L)(*[ptr(x) for x in xs])
    ya = (ctypes.c_void_p * L)(*[ptr(y) for y in ys])
    lib().ptc_cluster_center(ctypes.cast(xa, ctypes.c_void_p), ctypes.cast(perm, ctypes.c_void_p), ctypes.cast(ip, ctypes.c_void_p),
                             ctypes.cast(ncl, ctypes.c_void_p), L, n, c, dtype_code(xs[0]), ctypes.cast(ya, ctypes.c_void_p), stream_ptr())
    return ys


def cluster_agg_fwd(us: Sequence[torch.Tensor], vs: Sequence[torch.Tensor], a: torch.Tensor, gc: GridClusters):
    """out[n] = sum_l softmax(a[n])_l S_l[cluster_l[n]] (oacnns_v1m1_base.py:93-102) -> (out [N, C], state for the backward)."""
    require_cuda(*us, *vs, a)
    L = gc.levels
    if len(us) != L or len(vs) != L:
        raise PtcoreError(f"cluster_agg_fwd: {len(us)} / {len(vs)} tensors for {L} levels")
    n, c = us[0].shape
    dt = us[0].dtype
    _agg_rows(us, n, c, dt, "cluster_agg_fwd")
    _agg_rows(vs, n, c, dt, "cluster_agg_fwd")
    if a.dtype != dt or a.shape != (n, L) or not a.is_contiguous():
        raise PtcoreError(f"cluster_agg_fwd: a must be contiguous [{n}, {L}] {dt}, got {tuple(a.shape)} {a.dtype}")
    tot = sum(gc.n_cluster)
    sbytes = lib().ptc_cluster_agg_state_bytes(tot, c)
    state = torch.empty(sbytes, dtype=torch.uint8, device=a.device)
    out = torch.empty((n, c), dtype=dt, device=a.device)
    perm, ip, cl, ncl = gc._arrays()
    ua = (ctypes.c_void_p * L)(*[ptr(t) for t in us])
    va = (ctypes.c_void_p * L)(*[ptr(t) for t in vs])
    V = ctypes.c_void_p
    lib().ptc_cluster_agg_fwd(ctypes.cast(ua, V), ctypes.cast(va, V), ptr(a), ctypes.cast(perm, V), ctypes.cast(ip, V), ctypes.cast(cl, V),
                              ctypes.cast(ncl, V), L, n, c, dtype_code(a), ptr(out), ptr(state), sbytes, stream_ptr())
    return out, state


def cluster_agg_bwd(us, vs, a, dout: torch.Tensor, state: torch.Tensor, gc: GridClusters):
    """-> (du list, dv list, da): the gradients of cluster_agg_fwd, bit-reproducible (no float atomics)."""
    require_cuda(*us, *vs, a, dout, state)
    L = gc.levels
    n, c = us[0].shape
    dt = us[0].dtype
    dout = dout.to(dt).contiguous()
    _agg_rows([dout], n, c, dt, "cluster_agg_bwd")
    tot = sum(gc.n_cluster)
    du = [torch.empty_like(t) for t in us]
    dv = [torch.empty_like(t) for t in vs]
    da = torch.empty_like(a)
    wbytes = lib().ptc_cluster_agg_workspace_bytes(tot)
    ws = _ws(wbytes, a.device)
    perm, ip, cl, ncl = gc._arrays()
    V = ctypes.c_void_p
    keep = [(V * L)(*[ptr(t) for t in ts]) for ts in (us, vs, du, dv)]
    lib().ptc_cluster_agg_bwd(ctypes.cast(keep[0], V), ctypes.cast(keep[1], V), ptr(a), ptr(dout), ctypes.cast(perm, V), ctypes.cast(ip, V),
                              ctypes.cast(cl, V), ctypes.cast(ncl, V), L, n, c, dtype_code(a), ptr(state), state.numel(),
                              ctypes.cast(keep[2], V), ctypes.cast(keep[3], V), ptr(da), ptr(ws), wbytes, stream_ptr())
    return du, dv, da


# ------------------------------------------------------------------------------------------------
# PointGroup clustering and heads (csrc/pg_cluster.hip)
# ------------------------------------------------------------------------------------------------
PG_MAX_NEIGHBOURS = _K["PTC_PG_MAX_NEIGHBOURS"]


def pg_ball_query(xyz: torch.Tensor, batch_idxs: torch.Tensor, n_batch: int, radius: float):
    """ballquery_batch_p (bfs_cluster_kernel.cu:16-61) -> (idx [nActive] int32, start_len [n, 2] int32, n_truncated).
    Neighbours in ascending index order, the first 1000 of each point; sized exactly (ONE host read: nActive)."""
    require_cuda(xyz, batch_idxs)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise PtcoreError(f"pg_ball_query: xyz must be [n, 3], got {tuple(xyz.shape)}")
    x = xyz.float().contiguous()
    b = batch_idxs.to(torch.int32).contiguous()
    n = x.shape[0]
    if b.numel() != n:
        raise PtcoreError("pg_ball_query: batch_idxs must have one entry per point")
    dev = x.device
    start_len = torch.empty((n, 2), dtype=torch.int32, device=dev)
    total = torch.empty(2, dtype=torch.int64, device=dev)
    nbytes = lib().ptc_pg_ball_query_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    lib().ptc_pg_ball_query_count(ptr(x), ptr(b), n, int(n_batch), float(radius), ptr(start_len), ptr(total), ptr(ws), nbytes,
                                  stream_ptr())
    n_active, n_trunc = [int(v) for v in total.tolist()]
    if n_active >= 1 << 31:
        raise PtcoreError(f"pg_ball_query: {n_active} neighbour entries exceed the int32 index range")
    idx = torch.empty(n_active, dtype=torch.int32, device=dev)
    if n_active == 0:
        return idx, start_len, n_trunc
    lib().ptc_pg_ball_query_fill(ptr(x), n, float(radius), ptr(start_len), ptr(idx), ptr(ws), nbytes, stream_ptr())
    return idx, start_len, n_trunc


def pg_cluster(label: torch.Tensor, idx: torch.Tensor, start_len: torch.Tensor, threshold: int, skip_negative: bool = False):
    """bfs_cluster (bfs_cluster.cpp:53-145) -> (cluster_idxs [sumNPoint, 2] int32, cluster_offsets [nCluster + 1] int32), on the
    device; clusters in seed order, members in ascending point order (ONE host read: the two counts).  skip_negative: no cluster
    is seeded at a point with a negative label."""
    require_cuda(label, idx, start_len)
    lab = label.to(torch.int32).contiguous()
    ix = idx.to(torch.int32).contiguous()
    sl = start_len.to(torch.int32).contiguous()
    n = sl.shape[0]
    if sl.dim() != 2 or sl.shape[1] != 2 or lab.numel() != n:
        raise PtcoreError("pg_cluster: start_len must be [n, 2] and label [n]")
    dev = sl.device
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    nbytes = lib().ptc_pg_cluster_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    lib().ptc_pg_cluster_count(ptr(lab), ptr(ix), ptr(sl), n, int(threshold), int(bool(skip_negative)), ptr(counts), ptr(ws), nbytes, stream_ptr())
    n_cluster, n_sum = [int(v) for v in counts.tolist()]
    cidx = torch.empty((n_sum, 2), dtype=torch.int32, device=dev)
    coff = torch.empty(n_cluster + 1, dtype=torch.int32, device=dev)
    lib().ptc_pg_cluster_fill(n, n_cluster, n_sum, ptr(cidx), ptr(coff), ptr(ws), nbytes, stream_ptr())
    return cidx, coff


def pg_proposal_scores(logits: torch.Tensor, label: torch.Tensor, cluster_idxs: torch.Tensor, cluster_offsets: torch.Tensor,
                       point_map: Optional[torch.Tensor] = None):
    """per cluster: (count int32, class = label[seed] int32, mean softmax(logits)[member, class] fp32); members' logit rows are
    point_map[member] (or member)."""
    require_cuda(logits, label, cluster_idxs, cluster_offsets)
    lg = logits.contiguous()
    if lg.dim() != 2 or lg.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise PtcoreError(f"pg_proposal_scores: logits must be [n, c] fp32 / bf16 / f16, got {tuple(lg.shape)} {lg.dtype}")
    k = cluster_offsets.numel() - 1
    dev = lg.device
    count = torch.empty(k, dtype=torch.int32, device=dev)
    cls = torch.empty(k, dtype=torch.int32, device=dev)
    score = torch.empty(k, dtype=torch.float32, device=dev)
    pm = None if point_map is None else point_map.to(torch.int64).contiguous()
    lib().ptc_pg_proposal_scores(ptr(lg), dtype_code(lg), lg.shape[0], lg.shape[1], ptr(label.to(torch.int32).contiguous()),
                                 ptr(cluster_idxs.contiguous()), ptr(cluster_offsets.contiguous()), k, ptr(pm), ptr(count), ptr(cls),
                                 ptr(score), stream_ptr())
    return count, cls, score


def pg_proposal_masks(cluster_idxs: torch.Tensor, row: torch.Tensor, n_rows: int, n_points: int, point_map: Optional[torch.Tensor] = None):
    """dense [n_rows, n_points] int32 masks: 1 at (row[cluster], point_map[point]) for every member of a cluster with row >= 0"""
    require_cuda(cluster_idxs, row)
    out = torch.empty((int(n_rows), int(n_points)), dtype=torch.int32, device=cluster_idxs.device)
    pm = None if point_map is None else point_map.to(torch.int64).contiguous()
    ci = cluster_idxs.contiguous()
    lib().ptc_pg_proposal_masks(ptr(ci), ci.shape[0], ptr(row.to(torch.int64).contiguous()), ptr(pm), int(n_points), int(n_rows),
                                ptr(out), stream_ptr())
    return out


def _pg_bias_args(bias_pred, coord, centroid, instance):
    require_cuda(bias_pred, coord, centroid, instance)
    if bias_pred.dim() != 2 or bias_pred.shape[1] != 3 or bias_pred.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise PtcoreError(f"pg_bias_loss: bias_pred must be [n, 3] fp32 / bf16 / f16, got {tuple(bias_pred.shape)} {bias_pred.dtype}")
    n = bias_pred.shape[0]
    c = coord.float().contiguous()
    g = centroid.float().contiguous()
    i = instance.to(torch.int64).contiguous()
    if c.shape != (n, 3) or g.shape != (n, 3) or i.numel() != n:
        raise PtcoreError("pg_bias_loss: coord / instance_centroid must be [n, 3] and instance [n]")
    return bias_pred.contiguous(), c, g, i, n


def pg_bias_loss_fwd(bias_pred, coord, centroid, instance, ignore_index: int) -> torch.Tensor:
    """-> [3] fp32: (bias_l1_loss, bias_cosine_loss, sum(mask)) of point_group_v1m1_base.py:72-91"""
    bp, c, g, i, n = _pg_bias_args(bias_pred, coord, centroid, instance)
    out = torch.empty(3, dtype=torch.float32, device=bp.device)
    nbytes = lib().ptc_pg_bias_loss_workspace_bytes(n)
    ws = _ws(nbytes, bp.device)
    lib().ptc_pg_bias_loss_fwd(ptr(bp), dtype_code(bp), ptr(c), ptr(g), ptr(i), n, int(ignore_index), ptr(out), ptr(ws), nbytes,
                               stream_ptr())
    return out


def pg_bias_loss_bwd(bias_pred, coord, centroid, instance, ignore_index: int, dout: torch.Tensor, fwd_out: torch.Tensor) -> torch.Tensor:
    """d bias_pred [n, 3] (bias_pred's dtype) from dout [2] fp32 = (d l1, d cos)"""
    bp, c, g, i, n = _pg_bias_args(bias_pred, coord, centroid, instance)
    d = torch.empty_like(bp)
    lib().ptc_pg_bias_loss_bwd(ptr(bp), dtype_code(bp), ptr(c), ptr(g), ptr(i), n, int(ignore_index),
                               ptr(dout.float().contiguous()), ptr(fwd_out), ptr(d), stream_ptr())
    return d


# ------------------------------------------------------------------------------------------------
# Masked Scene Contrast (csrc/msc.hip)
# ------------------------------------------------------------------------------------------------
MSC_MAX_K = _K["PTC_MSC_MAX_K"]


def _msc_offsets(offset, new_offset, what):
    off, noff = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    if off.numel() != noff.numel() or off.numel() == 0:
        raise PtcoreError(f"{what}: both views must list the same (non-zero) number of scenes")
    return off, noff


def msc_match(k: int, max_radius: float, xyz, offset, new_xyz, new_offset):
    """For each row of new_xyz (view 1) the up-to-k points of its scene of xyz (view 2) with fp32 sqrt(d2) < max_radius, ascending
    (distance, index): knn_query(k, ...) followed by `dist < max_radius` (masked_scene_contrast_v1m1_base.py:147-162), found in the
    27 grid cells around the query.  -> (count [m] int32, cand [m, k] int32 with -1 padding, stats [2] int32 on the device:
    matched queries, largest count).  No host read."""
    require_cuda(xyz, offset, new_xyz, new_offset)
    x, q = _xyz(xyz, "xyz"), _xyz(new_xyz, "new_xyz")
    off, noff = _msc_offsets(offset, new_offset, "msc_match")
    n, m, dev = x.shape[0], q.shape[0], q.device
    count = torch.empty(m, dtype=torch.int32, device=dev)
    cand = torch.empty((m, int(k)), dtype=torch.int32, device=dev)
    stats = torch.empty(2, dtype=torch.int32, device=dev)
    nbytes = lib().ptc_msc_match_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    lib().ptc_msc_match(ptr(x), ptr(off), ptr(q), ptr(noff), off.numel(), n, m, int(k), float(max_radius), ptr(count), ptr(cand),
                        ptr(stats), ptr(ws), nbytes, stream_ptr())
    return count, cand, stats


def msc_select(count: torch.Tensor, cand: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """match_index [len(r), 2] int64 of :154-169: the j-th matched query q (ascending) with candidate count[q] - 1 - r[j] % count[q];
    len(r) must be the number of matched queries (stats[0] of msc_match)."""
    require_cuda(count, cand, r)
    cnt, cd = count.to(torch.int32).contiguous(), cand.to(torch.int32).contiguous()
    rr = r.to(torch.int64).contiguous()
    m, k = cd.shape
    if cnt.numel() != m or rr.dim() != 1:
        raise PtcoreError("msc_select: count must be [m], cand [m, k] and r [n_matched]")
    out = torch.empty((rr.numel(), 2), dtype=torch.int64, device=cd.device)
    nbytes = lib().ptc_msc_select_workspace_bytes(m)
    ws = _ws(nbytes, cd.device)
    lib().ptc_msc_select(ptr(cnt), ptr(cd), m, k, ptr(rr), rr.numel(), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


def msc_patch_rank(cell1, offset1, cell2, offset2):
    """cell1 / cell2 [n, 3] fp32 = floor(origin_coord / mask_grid_size) of the two views -> (cluster [n1 + n2] int32, view 1 first:
    the rank of each point's voxel_grid(pos=cell, size=1, batch, start=0) id over the union of both views in torch.unique's sorted
    order; patch_num [1] int64 on the device)."""
    require_cuda(cell1, offset1, cell2, offset2)
    c1, c2 = _xyz(cell1, "cell1"), _xyz(cell2, "cell2")
    o1, o2 = _msc_offsets(offset1, offset2, "msc_patch_rank")
    n1, n2, dev = c1.shape[0], c2.shape[0], c1.device
    cluster = torch.empty(n1 + n2, dtype=torch.int32, device=dev)
    patch_num = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = lib().ptc_msc_patch_workspace_bytes(n1 + n2)
    ws = _ws(nbytes, dev)
    lib().ptc_msc_patch_rank(ptr(c1), ptr(o1), n1, ptr(c2), ptr(o2), n2, o1.numel(), ptr(cluster), ptr(patch_num), ptr(ws), nbytes,
                             stream_ptr())
    return cluster, patch_num


def msc_patch_masks(cluster: torch.Tensor, patch_mask: torch.Tensor, n1: int):
    """(view1_point_mask [n1] bool, view2_point_mask bool) = (patch_mask[cluster] == 1, == 2) of :118-140"""
    require_cuda(cluster, patch_mask)
    cl, pm = cluster.to(torch.int32).contiguous(), patch_mask.to(torch.int32).contiguous()
    n2 = cl.numel() - int(n1)
    if n2 < 0:
        raise PtcoreError("msc_patch_masks: n1 exceeds the number of points")
    m1 = torch.empty(int(n1), dtype=torch.uint8, device=cl.device)
    m2 = torch.empty(n2, dtype=torch.uint8, device=cl.device)
    lib().ptc_msc_patch_masks(ptr(cl), ptr(pm), pm.numel(), int(n1), n2, ptr(m1), ptr(m2), stream_ptr())
    return m1.view(torch.bool), m2.view(torch.bool)


def msc_cross_masks(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset, mask_grid_size: float, mask_rate: float,
                    rand_perm=None):
    """generate_cross_masks (:69-141) -> (view1_point_mask, view2_point_mask) bool.  The patches are the voxel_grid ids of
    floor(origin / mask_grid_size) over the union of both views, ranked as torch.unique ranks them; rand_perm(patch_num) -> the
    permutation of the patches (default torch.randperm, as there).  ONE host read (patch_num); no [patch_num, patch_max_point] map."""
    if not mask_rate <= 0.5:
        raise PtcoreError("msc_cross_masks: mask_rate must be <= 0.5")
    c1 = torch.floor(view1_origin_coord.float().div(mask_grid_size))
    c2 = torch.floor(view2_origin_coord.float().div(mask_grid_size))
    cluster, patch_num = msc_patch_rank(c1, view1_offset, c2, view2_offset)
    patch_num = int(patch_num.item())
    perm = (torch.randperm if rand_perm is None else rand_perm)(patch_num)
    k = int(patch_num * mask_rate)
    patch_mask = torch.zeros(patch_num, dtype=torch.int32)
    patch_mask[perm[0:k]] = 1
    patch_mask[perm[k:k * 2]] = 2
    return msc_patch_masks(cluster, patch_mask.to(cluster.device), c1.shape[0])


def _msc_nce_args(feat1, feat2, match_index):
    require_cuda(feat1, feat2, match_index)
    if feat1.dtype != torch.float32 or feat2.dtype != torch.float32 or feat1.dim() != 2 or feat2.dim() != 2 or feat1.shape[1] != feat2.shape[1]:
        raise PtcoreError("msc_nce: feat1 / feat2 must be fp32 [N, C] with equal C")
    c = feat1.shape[1]
    mi = match_index.to(torch.int64).contiguous()
    if mi.dim() != 2 or mi.shape[1] != 2 or mi.shape[0] < 1:
        raise PtcoreError("msc_nce: match_index must be [P, 2] with P >= 1")
    return feat1.contiguous(), feat2.contiguous(), mi, c


def msc_nce_fwd(feat1, feat2, match_index, nce_t: float):
    """-> (out [3] fp32 = (nce loss, pos_sim, neg_sim) of :179-193, state for msc_nce_bwd); the P x P similarity matrix is never stored"""
    f1, f2, mi, c = _msc_nce_args(feat1, feat2, match_index)
    p, dev = mi.shape[0], f1.device
    an = torch.empty((p, c), dtype=torch.float32, device=dev)
    bn = torch.empty((p, c), dtype=torch.float32, device=dev)
    vec = torch.empty((3, p), dtype=torch.float32, device=dev)        # |a|, |b|, lse
    out = torch.empty(3, dtype=torch.float32, device=dev)
    nbytes = lib().ptc_msc_nce_workspace_bytes(p, c)
    ws = _ws(nbytes, dev)
    lib().ptc_msc_nce_fwd(ptr(f1), f1.shape[0], ptr(f2), f2.shape[0], ptr(mi), p, c, float(nce_t), ptr(an), ptr(bn), ptr(vec[0]),
                          ptr(vec[1]), ptr(vec[2]), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out, (an, bn, vec, mi)


def msc_nce_bwd(state, n1: int, n2: int, nce_t: float, dloss: torch.Tensor):
    """(dfeat1 [n1, C], dfeat2 [n2, C]) fp32 from the forward's state and d loss (a device scalar: no host read)"""
    an, bn, vec, mi = state
    p, c = an.shape
    dev = an.device
    d1 = torch.zeros((int(n1), c), dtype=torch.float32, device=dev)
    d2 = torch.zeros((int(n2), c), dtype=torch.float32, device=dev)
    g = dloss.to(torch.float32).reshape(1).contiguous()
    nbytes = lib().ptc_msc_nce_workspace_bytes(p, c)
    ws = _ws(nbytes, dev)
    lib().ptc_msc_nce_bwd(ptr(an), ptr(bn), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(mi), p, c, int(n1), int(n2), float(nce_t),
                          ptr(g), ptr(d1), ptr(d2), ptr(ws), nbytes, stream_ptr())
    return d1, d2


def _msc_csc_nce_args(feat1, coord1, offset1, feat2, coord2, match_index, r1, r2):
    require_cuda(feat1, coord1, offset1, feat2, coord2, match_index)
    if feat1.dtype != torch.float32 or feat2.dtype != torch.float32 or feat1.dim() != 2 or feat2.dim() != 2 or feat1.shape[1] != feat2.shape[1]:
        raise PtcoreError("msc_csc_nce: feat1 / feat2 must be fp32 [N, C] with equal C")
    c = feat1.shape[1]
    mi = match_index.to(torch.int64).contiguous()
    if mi.dim() != 2 or mi.shape[1] != 2 or mi.shape[0] < 1:
        raise PtcoreError("msc_csc_nce: match_index must be [P, 2] with P >= 1")
    x1, x2 = _xyz(coord1, "msc_csc_nce: coord1"), _xyz(coord2, "msc_csc_nce: coord2")
    if x1.shape[0] != feat1.shape[0] or x2.shape[0] != feat2.shape[0]:
        raise PtcoreError("msc_csc_nce: one coordinate row per feature row")
    off = offset1.to(torch.int32).contiguous()
    if off.dim() != 1 or off.numel() < 1:
        raise PtcoreError("msc_csc_nce: offset1 must list at least one scene")
    if not float(r1) <= float(r2):
        raise PtcoreError(f"msc_csc_nce: needs r1 <= r2, got r1={r1} r2={r2}")
    return feat1.contiguous(), x1, off, feat2.contiguous(), x2, mi, c


def msc_csc_nce_fwd(feat1, coord1, offset1, feat2, coord2, match_index, nce_t: float, r1: float, r2: float, partitions: int = 4):
    """-> (out [3] fp32 = (nce loss, pos_sim, neg_sim) of masked_scene_contrast_v1m2_csc.py:212-254, counts [nB, 5] int64 = the members
    of each partition class per scene, state for msc_csc_nce_bwd).  match_index in any order; no P x P matrix and no host read"""
    f1, x1, off, f2, x2, mi, c = _msc_csc_nce_args(feat1, coord1, offset1, feat2, coord2, match_index, r1, r2)
    p, nb, dev = mi.shape[0], off.numel(), f1.device
    an = torch.empty((p, c), dtype=torch.float32, device=dev)
    bn = torch.empty((p, c), dtype=torch.float32, device=dev)
    vec = torch.empty((3, p), dtype=torch.float32, device=dev)        # |a|, |b|, 1 / (nB partitions P_b)
    xs = torch.empty((2, p, 4), dtype=torch.float32, device=dev)      # (x1, scene), (x2, scene) in scene order
    smi = torch.empty((p, 2), dtype=torch.int64, device=dev)
    start = torch.empty(nb + 2, dtype=torch.int32, device=dev)
    lse = torch.empty((3, p, 5), dtype=torch.float32, device=dev)     # lse, row max, 1 / row sum, per class
    counts = torch.empty((nb, 5), dtype=torch.int64, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    nbytes = lib().ptc_msc_csc_nce_workspace_bytes(p, c, nb)
    ws = _ws(nbytes, dev)
    lib().ptc_msc_csc_nce_fwd(ptr(f1), f1.shape[0], ptr(f2), f2.shape[0], ptr(x1), ptr(x2), ptr(off), nb, ptr(mi), p, c, float(nce_t),
                              float(r1), float(r2), int(partitions), ptr(an), ptr(bn), ptr(vec[0]), ptr(vec[1]), ptr(xs[0]), ptr(xs[1]),
                              ptr(smi), ptr(start), ptr(lse[0]), ptr(lse[1]), ptr(lse[2]), ptr(vec[2]), ptr(counts), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out, counts, (an, bn, vec, xs, smi, start, lse)


def msc_csc_nce_bwd(state, n1: int, n2: int, nce_t: float, r1: float, r2: float, dloss: torch.Tensor):
    """(dfeat1 [n1, C], dfeat2 [n2, C]) fp32 from the forward's state and d loss (a device scalar: no host read)"""
    an, bn, vec, xs, smi, start, lse = state
    p, c = an.shape
    nb, dev = start.numel() - 2, an.device
    if not float(r1) <= float(r2):
        raise PtcoreError(f"msc_csc_nce: needs r1 <= r2, got r1={r1} r2={r2}")
    d1 = torch.zeros((int(n1), c), dtype=torch.float32, device=dev)
    d2 = torch.zeros((int(n2), c), dtype=torch.float32, device=dev)
    g = dloss.to(torch.float32).reshape(1).contiguous()
    nbytes = lib().ptc_msc_csc_nce_workspace_bytes(p, c, nb)
    ws = _ws(nbytes, dev)
    lib().ptc_msc_csc_nce_bwd(ptr(an), ptr(bn), ptr(vec[0]), ptr(vec[1]), ptr(xs[0]), ptr(xs[1]), ptr(smi), ptr(start), ptr(lse[1]),
                              ptr(lse[2]), ptr(vec[2]), p, c, nb, int(n1), int(n2), float(nce_t), float(r1), float(r2), ptr(g), ptr(d1), ptr(d2),
                              ptr(ws), nbytes, stream_ptr())
    return d1, d2


# ------------------------------------------------------------------------------------------------
# context-aware classifier (csrc/cac.hip): prototype pooling, segmented cosine classifier, distillation loss
# ------------------------------------------------------------------------------------------------
def cac_supported(k: int, c: int) -> bool:
    return bool(lib().ptc_cac_supported(int(k), int(c)))


def _cac_rows(x: torch.Tensor, what: str) -> torch.Tensor:
    require_cuda(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise PtcoreError(f"{what}: needs fp32 [N, C] rows, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def _cac_offset(offset, device):
    if offset is None:
        return None, 1
    o = offset.to(device=device, dtype=torch.int64).contiguous()
    return o, int(o.numel())


def cac_pool_fwd(x, logits=None, target=None, offset=None, num_classes=None, conf_thresh: float = 0.0, eps: float = 1e-7):
    """-> (proto [S, K, C], wsum [S, K], count [K] int64 | None, passed [S] int64).  logits [N, K]: w_i = softmax(logits_i) times the
    confidence gate, rows segmented by `offset`; target [N] (needs num_classes): w_i = onehot(target_i), one segment, count = the
    class counts.  proto = sum_i w_ik x_i / (sum_i w_ik + eps); the weights are never written to memory."""
    x = _cac_rows(x, "cac_pool_fwd")
    n, c = x.shape
    hard = target is not None
    if hard == (logits is not None):
        raise PtcoreError("cac_pool_fwd: exactly one of logits / target")
    if hard:
        require_cuda(target)
        target = target.to(torch.int64).contiguous()
        k, off, s = int(num_classes), None, 1
    else:
        logits = _cac_rows(logits, "cac_pool_fwd")
        k = logits.shape[1]
        off, s = _cac_offset(offset, x.device)
    dev = x.device
    proto = torch.empty((s, k, c), dtype=torch.float32, device=dev)
    wsum = torch.empty((s, k), dtype=torch.float32, device=dev)
    count = torch.empty(k, dtype=torch.int64, device=dev) if hard else None
    passed = torch.empty(s, dtype=torch.int64, device=dev)
    nbytes = lib().ptc_cac_pool_workspace_bytes(n, s, k, c)
    ws = _ws(nbytes, dev)
    lib().ptc_cac_pool_fwd(ptr(x), ptr(logits), ptr(target), ptr(off), n, s, k, c, float(conf_thresh), float(eps), ptr(proto), ptr(wsum),
                           ptr(count), ptr(passed), ptr(ws), nbytes, stream_ptr())
    return proto, wsum, count, passed


def cac_pool_bwd(x, logits, target, offset, conf_thresh: float, eps: float, proto, wsum, dproto, need_dlogits: bool):
    """(dx [N, C], dlogits [N, K] | None) of cac_pool_fwd; the softmax rows are recomputed"""
    x = _cac_rows(x, "cac_pool_bwd")
    n, c = x.shape
    s, k = wsum.shape
    off, _ = _cac_offset(offset, x.device)
    dx = torch.empty_like(x)
    if logits is not None:
        logits = _cac_rows(logits, "cac_pool_bwd")
    dl = torch.empty_like(logits) if (need_dlogits and logits is not None) else None
    dp = dproto.to(torch.float32).contiguous()          # kept in a name: the copy must outlive the call
    lib().ptc_cac_pool_bwd(ptr(x), ptr(logits), ptr(target), ptr(off), n, s, k, c, float(conf_thresh), float(eps), ptr(proto), ptr(wsum),
                           ptr(dp), ptr(dx), ptr(dl), stream_ptr())
    return dx, dl


def cac_cos_fwd(x, proto, offset, cos_temp: float):
    """out [N, K] = cos_temp * normalize(x_i) . normalize(proto[s(i), k]); proto [S, K, C]"""
    x, p = _cac_rows(x, "cac_cos_fwd"), proto.contiguous()
    n, c = x.shape
    s, k = p.shape[0], p.shape[1]
    off, so = _cac_offset(offset, x.device)
    if p.dim() != 3 or p.shape[2] != c or p.dtype != torch.float32 or so != s:
        raise PtcoreError(f"cac_cos_fwd: prototypes {tuple(p.shape)} {p.dtype} for rows {tuple(x.shape)} in {so} segment(s)")
    out = torch.empty((n, k), dtype=torch.float32, device=x.device)
    nbytes = lib().ptc_cac_cos_workspace_bytes(n, s, k, c)
    ws = _ws(nbytes, x.device)
    lib().ptc_cac_cos_fwd(ptr(x), ptr(p), ptr(off), n, s, k, c, float(cos_temp), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


def cac_cos_bwd(x, proto, offset, cos_temp: float, dout):
    """(dx [N, C], dproto [S, K, C]) of cac_cos_fwd; dproto is reduced per segment in a fixed order"""
    x, p = _cac_rows(x, "cac_cos_bwd"), proto.contiguous()
    n, c = x.shape
    s, k = p.shape[0], p.shape[1]
    off, _ = _cac_offset(offset, x.device)
    dx, dp = torch.empty_like(x), torch.empty_like(p)
    nbytes = lib().ptc_cac_cos_workspace_bytes(n, s, k, c)
    ws = _ws(nbytes, x.device)
    do = dout.to(torch.float32).contiguous()            # kept in a name: the copy must outlive the call
    lib().ptc_cac_cos_bwd(ptr(x), ptr(p), ptr(off), n, s, k, c, float(cos_temp), ptr(do), ptr(dx), ptr(dp), ptr(ws), nbytes,
                          stream_ptr())
    return dx, dp


def cac_distill_fwd(pred, soft, target, smoothness: float, eps: float):
    """-> (loss [1], stats [3, K]) of get_distill_loss (:152-199); stats = per-class sums of loss * entropy, entropy, row counts"""
    pred, soft = _cac_rows(pred, "cac_distill_fwd"), _cac_rows(soft, "cac_distill_fwd")
    require_cuda(target)
    n, k = pred.shape
    if soft.shape != pred.shape or target.shape != (n,):
        raise PtcoreError(f"cac_distill_fwd: pred {tuple(pred.shape)}, soft {tuple(soft.shape)}, target {tuple(target.shape)}")
    tg = target.to(torch.int64).contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    stats = torch.empty((3, k), dtype=torch.float32, device=pred.device)
    nbytes = lib().ptc_cac_distill_workspace_bytes(n, k)
    ws = _ws(nbytes, pred.device)
    lib().ptc_cac_distill_fwd(ptr(pred), ptr(soft), ptr(tg), n, k, float(smoothness), float(eps), ptr(loss), ptr(stats), ptr(ws), nbytes,
                              stream_ptr())
    return loss, stats, (pred, soft, tg)


def cac_distill_bwd(state, smoothness: float, eps: float, stats, dloss):
    pred, soft, tg = state
    n, k = pred.shape
    dpred = torch.empty_like(pred)
    g = dloss.to(torch.float32).reshape(1).contiguous()
    lib().ptc_cac_distill_bwd(ptr(pred), ptr(soft), ptr(tg), n, k, float(smoothness), float(eps), ptr(stats), ptr(g), ptr(dpred),
                              stream_ptr())
    return dpred


# ------------------------------------------------------------------------------------------------
# Point Prompt Training's language-guided head (csrc/ppt.hip)
# ------------------------------------------------------------------------------------------------
def ppt_head_supported(c: int, d: int, k: int, dtype: torch.dtype) -> bool:
    return dtype in _DT and bool(lib().ptc_ppt_head_supported(int(c), int(d), int(k), _DT[dtype]))


def _ppt_f32(t: torch.Tensor, shape, what: str, dtype=torch.float32) -> torch.Tensor:
    require_cuda(t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise PtcoreError(f"{what}: needs {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def ppt_head_fwd(x, w, b, e, scale: float, eps: float):
    """-> (logits [N, K] fp32, inv_norm [N] fp32): logits = scale * (h e^T) / max(|h|, eps) with h = x w^T + b [N, D] formed and
    consumed in registers.  x [N, C] fp32 / bf16 / fp16, w [D, C] of x's dtype, b [D] and e [K, D] (the selected class rows) fp32."""
    require_cuda(x, w)
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1] or w.dtype != x.dtype:
        raise PtcoreError(f"ppt_head_fwd: x {x.dtype} {tuple(x.shape)}, w {w.dtype} {tuple(w.shape)}")
    x, w = x.contiguous(), w.contiguous()
    (n, c), d, k = x.shape, w.shape[0], e.shape[0]
    b, e = _ppt_f32(b, (d,), "ppt_head_fwd: b"), _ppt_f32(e, (k, d), "ppt_head_fwd: e")
    logits = torch.empty((n, k), dtype=torch.float32, device=x.device)
    inv = torch.empty(n, dtype=torch.float32, device=x.device)
    lib().ptc_ppt_head_fwd(ptr(x), ptr(w), ptr(b), ptr(e), n, c, d, k, dtype_code(x), float(scale), float(eps), ptr(logits), ptr(inv),
                           stream_ptr())
    return logits, inv


def ppt_head_bwd(x, dlogits, logits, inv_norm, G, M, u, d: int, scale: float, eps: float):
    """-> (dx [N, C] of x's dtype, A [K, C], Bm [C, C], v [C], asum [K], rsum [1]) of ppt_head_fwd from dlogits [N, K] and the small
    products G = e w [K, C] (fp32), M = w^T w [C, C], u = w^T b [C] (float64); the five reductions in a fixed order (csrc/ppt.hip)"""
    require_cuda(x)
    x = x.contiguous()
    n, c = x.shape
    k = logits.shape[1]
    dl = _ppt_f32(dlogits, (n, k), "ppt_head_bwd: dlogits")            # kept in names: the copies must outlive the call
    lg, iv = _ppt_f32(logits, (n, k), "ppt_head_bwd: logits"), _ppt_f32(inv_norm, (n,), "ppt_head_bwd: inv_norm")
    G = _ppt_f32(G, (k, c), "ppt_head_bwd: G")
    M, u = _ppt_f32(M, (c, c), "ppt_head_bwd: M", torch.float64), _ppt_f32(u, (c,), "ppt_head_bwd: u", torch.float64)
    dev = x.device
    dx = torch.empty_like(x)
    A, Bm = torch.empty((k, c), dtype=torch.float32, device=dev), torch.empty((c, c), dtype=torch.float32, device=dev)
    v, asum, rsum = (torch.empty(s, dtype=torch.float32, device=dev) for s in (c, k, 1))
    nbytes = lib().ptc_ppt_head_workspace_bytes(n, c, int(d), k)
    ws = _ws(nbytes, dev)
    lib().ptc_ppt_head_bwd(ptr(x), ptr(dl), ptr(lg), ptr(iv), ptr(G), ptr(M), ptr(u), n, c, int(d), k, dtype_code(x), float(scale), float(eps),
                           ptr(dx), ptr(A), ptr(Bm), ptr(v), ptr(asum), ptr(rsum), ptr(ws), nbytes, stream_ptr())
    return dx, A, Bm, v, asum, rsum


# ------------------------------------------------------------------------------------------------
# SGIFormer decoder (csrc/sgiformer.hip): ragged masked attention, mask bit-pack, matcher cost, target builder
# ------------------------------------------------------------------------------------------------
def sgi_attn_supported(d: int) -> bool:
    return bool(lib().ptc_sgi_attn_supported(int(d)))


def sgi_cu(lengths: Sequence[int], device) -> torch.Tensor:
    """int32 [S + 1] row starts of a ragged batch from its host lengths"""
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + int(n))
    return torch.tensor(cu, dtype=torch.int32, device=device)


def sgi_offsets(rows: Sequence[int], cols: Sequence[int], device, packed: bool):
    """(int64 [S + 1] starts, total) of per-scene [rows_i, cols_i] blocks laid end to end: in elements, or, `packed`, in the uint32
    words of one bit per element (ceil(cols_i / 32) words per row)"""
    off = [0]
    for r, c in zip(rows, cols):
        off.append(off[-1] + int(r) * ((int(c) + 31) // 32 if packed else int(c)))
    return torch.tensor(off, dtype=torch.int64, device=device), off[-1]


def _sgi_rows(x: torch.Tensor, what: str) -> torch.Tensor:
    require_cuda(x)
    if x.dim() != 3 or x.dtype not in (torch.float32, torch.bfloat16):
        raise PtcoreError(f"{what}: needs fp32 / bf16 [T, H, D] rows, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def sgi_attn_fwd(q, k, v, cu_q, cu_k, mask=None, mask_row_off=None, scale=None):
    """-> (out [Tq, H, D], lse [Tq, H] fp32).  Scene i attends rows cu_q[i]:cu_q[i+1] of q to rows cu_k[i]:cu_k[i+1] of k, v; `mask`
    int32 words, one bit per (query, key) of each scene from word mask_row_off[i], set = masked out, no row fully masked."""
    q, k, v = _sgi_rows(q, "sgi_attn_fwd"), _sgi_rows(k, "sgi_attn_fwd"), _sgi_rows(v, "sgi_attn_fwd")
    tq, h, d = q.shape
    tk = k.shape[0]
    if k.shape != v.shape or k.shape[1:] != q.shape[1:] or k.dtype != q.dtype or v.dtype != q.dtype:
        raise PtcoreError(f"sgi_attn_fwd: q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)} {k.dtype}, v {tuple(v.shape)} {v.dtype}")
    s = cu_q.numel() - 1
    if cu_k.numel() != s + 1 or cu_q.dtype != torch.int32 or cu_k.dtype != torch.int32:
        raise PtcoreError("sgi_attn_fwd: cu_q / cu_k must be int32 [S + 1]")
    scale = float(d) ** -0.5 if scale is None else float(scale)
    out = torch.empty_like(q)
    lse = torch.empty((tq, h), dtype=torch.float32, device=q.device)
    lib().ptc_sgi_attn_fwd(ptr(q), ptr(k), ptr(v), dtype_code(q), ptr(cu_q), ptr(cu_k), s, tq, tk, h, d, ptr(mask), ptr(mask_row_off), scale,
                           ptr(out), ptr(lse), stream_ptr())
    return out, lse


def sgi_attn_bwd(q, k, v, out, dout, lse, cu_q, cu_k, mask=None, mask_row_off=None, scale=None):
    """(dq, dk, dv) of sgi_attn_fwd; the probabilities are recomputed, the reductions run in a fixed order"""
    q, k, v = _sgi_rows(q, "sgi_attn_bwd"), _sgi_rows(k, "sgi_attn_bwd"), _sgi_rows(v, "sgi_attn_bwd")
    tq, h, d = q.shape
    tk = k.shape[0]
    s = cu_q.numel() - 1
    scale = float(d) ** -0.5 if scale is None else float(scale)
    do = dout.to(q.dtype).contiguous()                  # kept in a name: the copy must outlive the call
    o = out.contiguous()
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    nbytes = lib().ptc_sgi_attn_workspace_bytes(tq, h)
    ws = _ws(nbytes, q.device)
    lib().ptc_sgi_attn_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), dtype_code(q), ptr(cu_q), ptr(cu_k), s, tq, tk, h, d, ptr(mask),
                           ptr(mask_row_off), scale, ptr(dq), ptr(dk), ptr(dv), ptr(ws), nbytes, stream_ptr())
    return dq, dk, dv


def sgi_pack_mask(logits: torch.Tensor, lq: Sequence[int], lk: Sequence[int]):
    """-> (words int32 [total], row_off int64 [S + 1]).  logits: the [lq_i, lk_i] fp32 mask logits of every scene laid end to end;
    bit = sigmoid(x) < 0.5, a row whose bits would all be set is cleared (forward_head, :372-378)."""
    require_cuda(logits)
    if logits.dtype != torch.float32:
        raise PtcoreError(f"sgi_pack_mask: fp32 logits, got {logits.dtype}")
    x = logits.contiguous().reshape(-1)
    dev = x.device
    logit_off, total = sgi_offsets(lq, lk, dev, False)
    if total != x.numel():
        raise PtcoreError(f"sgi_pack_mask: {x.numel()} logits for blocks of {total}")
    row_off, nwords = sgi_offsets(lq, lk, dev, True)
    words = torch.empty(nwords, dtype=torch.int32, device=dev)
    cu_q, cu_k = sgi_cu(lq, dev), sgi_cu(lk, dev)
    lib().ptc_sgi_pack_mask(ptr(x), ptr(logit_off), ptr(cu_q), ptr(cu_k), len(lq), int(sum(lq)), ptr(row_off), ptr(words), stream_ptr())
    return words, row_off


def sgi_match_cost(logits: torch.Tensor, cls: torch.Tensor, lq: Sequence[int], lk: Sequence[int], g: Sequence[int], gt_words: torch.Tensor,
                   gt_word_off: torch.Tensor, gt_cls: torch.Tensor, weights: Sequence[float]):
    """-> (cost fp32 [sum lq_i g_i], cost_off host list [S + 1]): the Hungarian matcher's cost matrices [lq_i, g_i] of every scene
    (loss.py:15-52, :331-429) from the flat mask logits, cls [Tq, C] and the packed ground-truth masks [g_i, lk_i]."""
    require_cuda(logits, cls, gt_words, gt_cls)
    x = logits.to(torch.float32).contiguous().reshape(-1)
    c = cls.to(torch.float32).contiguous()
    dev = x.device
    logit_off, total = sgi_offsets(lq, lk, dev, False)
    if total != x.numel() or c.dim() != 2 or c.shape[0] != sum(lq):
        raise PtcoreError(f"sgi_match_cost: {x.numel()} logits for blocks of {total}, cls {tuple(c.shape)} for {sum(lq)} rows")
    cost_off, ncost = sgi_offsets(lq, g, dev, False)
    cost = torch.empty(ncost, dtype=torch.float32, device=dev)
    cu_q, cu_k, cu_g = sgi_cu(lq, dev), sgi_cu(lk, dev), sgi_cu(g, dev)
    gc = gt_cls.to(torch.int64).contiguous()
    if ncost:
        lib().ptc_sgi_match_cost(ptr(x), ptr(logit_off), ptr(c), c.shape[1], ptr(cu_q), ptr(cu_k), ptr(cu_g), len(lq), int(sum(lq)),
                                 ptr(gt_words), ptr(gt_word_off), ptr(gc), ptr(cost_off), float(weights[0]), float(weights[1]),
                                 float(weights[2]), ptr(cost), stream_ptr())
    off, host = 0, [0]
    for a, b in zip(lq, g):
        off += int(a) * int(b)
        host.append(off)
    return cost, host


def sgi_targets(instance, segment, sp_inverse, offset, lk: Sequence[int], g: Sequence[int]):
    """prepare_target (:517-585) without the [N, G] one-hot -> (sp_size int32 [sum lk], counts int32 [sum g_i lk_i], gt_words int32,
    word_off int64 [S + 1], inst_cls int64 [sum g_i]); g_i = max instance + 1 of scene i (0: none), lk_i its superpoints."""
    require_cuda(instance, segment, sp_inverse, offset)
    dev = instance.device
    inst = instance.to(torch.int64).contiguous()
    seg = segment.to(torch.int64).contiguous()
    spi = sp_inverse.to(torch.int64).contiguous()
    off = offset.to(torch.int64).contiguous()
    s, n = off.numel(), inst.numel()
    if len(lk) != s or len(g) != s:
        raise PtcoreError("sgi_targets: one superpoint and one instance count per scene")
    cu_k, cu_g = sgi_cu(lk, dev), sgi_cu(g, dev)
    cnt_off, ncnt = sgi_offsets(g, lk, dev, False)
    word_off, nwords = sgi_offsets(g, lk, dev, True)
    nsp, ninst = int(sum(lk)), int(sum(g))
    sp_size = torch.empty(nsp, dtype=torch.int32, device=dev)
    counts = torch.empty(ncnt, dtype=torch.int32, device=dev)
    words = torch.empty(nwords, dtype=torch.int32, device=dev)
    inst_cls = torch.empty(ninst, dtype=torch.int64, device=dev)
    lib().ptc_sgi_targets(ptr(inst), ptr(seg), ptr(spi), ptr(off), s, n, ptr(cu_k), ptr(cu_g), ptr(cnt_off), ptr(word_off), nsp, ninst, ncnt,
                          nwords, ptr(sp_size), ptr(counts), ptr(words), ptr(inst_cls), stream_ptr())
    return sp_size, counts, words, word_off, inst_cls


# ------------------------------------------------------------------------------------------------
# Sonata-v1m1 distillation loss (csrc/sonata.hip): Sinkhorn-Knopp in scaling-vector form and the fused soft cross entropy
# ------------------------------------------------------------------------------------------------
def sonata_supported(k: int) -> bool:
    """whether the kernels take K prototypes (ptc_sonata_supported states the rule: include/ptcore.h)"""
    return bool(lib().ptc_sonata_supported(int(k)))


def _sonata_rows(x, what):
    require_cuda(x)
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise PtcoreError(f"{what}: logits must be [N, K] in fp32, fp16 or bf16, got {tuple(x.shape)} {x.dtype}")
    if not sonata_supported(x.shape[1]):
        raise PtcoreError(f"{what}: K={x.shape[1]} prototypes are not served (ptc_sonata_supported, include/ptcore.h)")
    return x.detach().contiguous()


def _sonata_pairs(match_index, what):
    require_cuda(match_index)
    if match_index.dim() != 2 or match_index.shape[1] != 2:
        raise PtcoreError(f"{what}: match_index must be [M, 2]")
    return match_index.to(torch.int64).contiguous()


def _sonata_vec(v, n, what):
    require_cuda(v)
    if v.shape != (n,):
        raise PtcoreError(f"{what}: expected a vector of {n}, got {tuple(v.shape)}")
    return v.detach().to(torch.float32).contiguous()


def _sonata_partials(m: int, k: int, max_groups: int, device):
    return torch.empty((int(lib().ptc_sonata_groups(m, k, int(max_groups))), k), dtype=torch.float32, device=device)


def sonata_colsum(teacher_sim, match_index, temp: float, b=None, max_groups: int = 0):
    """r [K] fp32 = sum_i exp(teacher_sim[match_index[i, 1]] / temp) b_i (b = None: 1).  One partial row per workgroup (at most
    max_groups of them, 0 = the default) summed in index order: bit-reproducible.  Zeros for an empty match_index."""
    t, mi = _sonata_rows(teacher_sim, "sonata_colsum"), _sonata_pairs(match_index, "sonata_colsum")
    m, k = mi.shape[0], t.shape[1]
    r = torch.zeros(k, dtype=torch.float32, device=t.device)
    if m == 0:
        return r
    bb = None if b is None else _sonata_vec(b, m, "sonata_colsum")
    part = _sonata_partials(m, k, max_groups, t.device)
    lib().ptc_sonata_colsum(ptr(t), dtype_code(t), t.shape[0], ptr(mi), m, k, float(temp), ptr(bb), int(max_groups), ptr(part), ptr(r),
                            stream_ptr())
    return r


def sonata_rowpass(teacher_sim, match_index, temp: float, a, n: float, want_colsum: bool = True, max_groups: int = 0):
    """From the prototype scales a [K]: (c [M] = sum_k e_ik a_k, b [M] = 1 / (n c), r [K] = sum_i e_ik b_i or None) in one pass over
    the gathered teacher rows; n = the global number of rows."""
    t, mi = _sonata_rows(teacher_sim, "sonata_rowpass"), _sonata_pairs(match_index, "sonata_rowpass")
    m, k = mi.shape[0], t.shape[1]
    av = _sonata_vec(a, k, "sonata_rowpass")
    c = torch.zeros(m, dtype=torch.float32, device=t.device)
    b = torch.zeros(m, dtype=torch.float32, device=t.device)
    r = torch.zeros(k, dtype=torch.float32, device=t.device) if want_colsum else None
    if m == 0:
        return c, b, r
    part = _sonata_partials(m, k, max_groups, t.device) if want_colsum else None
    lib().ptc_sonata_rowpass(ptr(t), dtype_code(t), t.shape[0], ptr(mi), m, k, float(temp), ptr(av), float(n), ptr(c), ptr(b),
                             int(max_groups), ptr(part), ptr(r), stream_ptr())
    return c, b, r


def sonata_distill_fwd(teacher_sim, student_sim, match_index, student_batch, num_scenes: int, temp: float, student_temp: float, a,
                       max_groups: int = 0):
    """The last row pass fused with the loss (sonata_v1m1_base.py:443-454) -> (loss [1] fp32, scene_mean [num_scenes], state for
    sonata_distill_bwd).  num_scenes bounds student_batch; match_index must be non-empty and listed by ascending scene."""
    t, s = _sonata_rows(teacher_sim, "sonata_distill_fwd"), _sonata_rows(student_sim, "sonata_distill_fwd")
    mi = _sonata_pairs(match_index, "sonata_distill_fwd")
    m, k, dev = mi.shape[0], t.shape[1], t.device
    if s.shape[1] != k or m < 1:
        raise PtcoreError(f"sonata_distill_fwd: teacher K={k}, student K={s.shape[1]}, {m} pairs (at least one)")
    require_cuda(student_batch)
    sb = student_batch.to(torch.int64).contiguous()
    if sb.shape != (s.shape[0],):
        raise PtcoreError("sonata_distill_fwd: student_batch must list one scene per student row")
    av = _sonata_vec(a, k, "sonata_distill_fwd")
    vec = torch.zeros((4, m), dtype=torch.float32, device=dev)          # c, lse, row loss, row weight
    scene_mean = torch.zeros(int(num_scenes), dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    lib().ptc_sonata_distill_fwd(ptr(t), dtype_code(t), t.shape[0], ptr(s), dtype_code(s), s.shape[0], ptr(mi), ptr(sb), int(num_scenes), m,
                                 k, float(temp), float(student_temp), ptr(av), int(max_groups), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]),
                                 ptr(vec[3]), ptr(scene_mean), ptr(loss), stream_ptr())
    return loss, scene_mean, (t, s, mi, av, vec)


def sonata_distill_bwd(state, temp: float, student_temp: float, dloss, max_groups: int = 0):
    """d loss / d student_sim [Ns, K] in the student's dtype: matched rows written by the kernel, every other row exactly zero"""
    t, s, mi, av, vec = state
    dpred = torch.zeros_like(s)
    g = dloss.detach().to(torch.float32).reshape(1).contiguous()
    lib().ptc_sonata_distill_bwd(ptr(t), dtype_code(t), t.shape[0], ptr(s), dtype_code(s), s.shape[0], ptr(mi), mi.shape[0], t.shape[1],
                                 float(temp), float(student_temp), ptr(av), ptr(vec[0]), ptr(vec[1]), ptr(vec[3]), ptr(g),
                                 int(max_groups), ptr(dpred), stream_ptr())
    return dpred


def sonata_patch_rank(grid_coord: torch.Tensor, batch: torch.Tensor, n_batch: int):
    """generate_mask's point_cluster (sonata_v1m1_base.py:298-304): the rank of every point's (batch, cell) row among the sorted
    unique rows, = torch.unique(cat([batch, grid_coord]), dim=0, sorted=True, return_inverse=True)[1], by one key sort and the
    run-numbering kernel of the pooling maps.  grid_coord [N, 3] >= 0.  -> (cluster [N] int64, facts [2] int64 ON THE DEVICE:
    the number of patches, and non-zero when a cell does not fit the key) -- the caller reads both in its one host read."""
    require_cuda(grid_coord, batch)
    n = grid_coord.shape[0]
    bb = max(1, (int(n_batch) - 1).bit_length())
    cb = min(20, (62 - bb) // 3)
    gl = grid_coord.to(torch.int64)
    key = ((((batch.to(torch.int64) << cb) | gl[:, 0]) << cb | gl[:, 1]) << cb | gl[:, 2]).contiguous()
    order, _ = sort_keys(key[None].contiguous(), 0, 3 * cb + bb, want_inverse=False)
    order0 = order[0].contiguous()
    cluster = torch.empty(n, dtype=torch.int64, device=key.device)
    ncl = torch.empty(1, dtype=torch.int64, device=key.device)
    nbytes = lib().ptc_pool_maps_workspace_bytes(n)
    ws = _ws(nbytes, key.device)
    lib().ptc_pool_maps_count(ptr(key), ptr(order0), n, 0, ptr(cluster), ptr(ncl), ptr(ws), nbytes, stream_ptr())
    bad = ((gl.amax() >> cb) != 0) | (gl.amin() < 0) if n else ncl.new_zeros(())
    return cluster, torch.stack([ncl[0], bad.to(torch.int64)])


# ------------------------------------------------------------------------------------------------
# Concerto-v1m1 2D-3D alignment branch (csrc/concerto.hip)
# ------------------------------------------------------------------------------------------------
_CONCERTO_CORR_TYPES = {torch.float32: _K["PTC_CORR_F32"], torch.int32: _K["PTC_CORR_I32"], torch.int64: _K["PTC_CORR_I64"]}


def concerto_pool_corr(corr: torch.Tensor, perm: Optional[torch.Tensor], idx_ptr: torch.Tensor) -> torch.Tensor:
    """Concerto.pool_corr (concerto_v1m1_base.py:545-570) for one pooling level and all images in one launch: corr [N, V, 2] (fp32,
    int32 or int64), perm = the points sorted by cluster, idx_ptr [M + 1] -> [M, V, 2] fp32.  Per (cluster, image): sum over all
    members with -1 read as 0, component by component, divided by the number of members with both components != -1; (-1, -1) where
    that number is 0.  Members are summed in CSR order in double.  V == 0: an empty [M, 0, 2], no launch."""
    require_cuda(corr, perm, idx_ptr)
    if corr.dim() != 3 or corr.shape[2] != 2 or corr.dtype not in _CONCERTO_CORR_TYPES:
        raise PtcoreError(f"concerto_pool_corr: correspondence must be [N, V, 2] in fp32, int32 or int64, got {tuple(corr.shape)} {corr.dtype}")
    n, v = corr.shape[0], corr.shape[1]
    m = idx_ptr.numel() - 1
    out = torch.empty((m, v, 2), dtype=torch.float32, device=corr.device)
    if m == 0 or v == 0:
        return out
    corr = corr.contiguous()
    idx_ptr = idx_ptr.to(torch.int64).contiguous()
    perm = None if perm is None else perm.to(torch.int64).contiguous()
    if perm is not None and perm.numel() < n:
        raise PtcoreError("concerto_pool_corr: perm is shorter than the points")
    lib().ptc_concerto_pool_corr(ptr(corr), _CONCERTO_CORR_TYPES[corr.dtype], n, v, ptr(perm), ptr(idx_ptr), m, ptr(out), stream_ptr())
    return out


class ConcertoPairs:
    """The (point, image) pairs of the alignment branch grouped by image patch: patch_ids [U] (sorted unique), indptr [U + 1] over the
    pairs in (patch, point row, view) order, perm [P] = the feature row of every pair in that order, pair_patch [Ns, V] = the patch
    (index into patch_ids) of every pair or -1, rows [Ns] = the feature row of every selected point (None: identity)."""

    def __init__(self, patch_ids, indptr, perm, pair_patch, rows):
        self.patch_ids, self.indptr, self.perm, self.pair_patch, self.rows = patch_ids, indptr, perm, pair_patch, rows

    @property
    def num_patches(self) -> int:
        return int(self.patch_ids.numel())

    @property
    def num_pairs(self) -> int:
        return int(self.perm.numel())


def concerto_patch_pairs(corr: torch.Tensor, scene: torch.Tensor, img_offset: torch.Tensor, img_num: torch.Tensor, total_images: int,
                         patch_h: int, patch_w: int, rows: Optional[torch.Tensor] = None) -> ConcertoPairs:
    """The patch binning of :786-830 without the dense tensor.  corr [N, V, 2] fp32 pooled correspondence, rows [Ns] the selected
    points (None: all), scene [Ns] their scene, img_offset / img_num [B] the first image and the image count of every scene,
    total_images = img_num.sum() (host).  A pair (point, view) with any(corr != -1) gets the key
    (img_offset[scene] + view) * patch_h * patch_w + trunc(row) * patch_w + trunc(col); one key sort (ops.sort_keys) and the
    run-numbering kernels of the pooling maps give the sorted unique ids -- torch.unique's order -- and the CSR, pairs inside a patch
    by ascending point row, then view.  One host read (the number of patches and of pairs).
    DIFFERENCE FROM THE REFERENCE: a pair whose truncated row or column lies outside [0, patch_h) x [0, patch_w), or whose view is at
    or beyond its scene's img_num, aliases into another image's patches there; here it is left out."""
    require_cuda(corr, scene, img_offset, img_num, rows)
    if corr.dim() != 3 or corr.shape[2] != 2 or corr.dtype != torch.float32:
        raise PtcoreError(f"concerto_patch_pairs: pooled correspondence must be [N, V, 2] fp32, got {tuple(corr.shape)} {corr.dtype}")
    dev = corr.device
    n, v = corr.shape[0], corr.shape[1]
    rows = None if rows is None else rows.to(torch.int64).contiguous()
    ns = n if rows is None else rows.numel()
    if scene.numel() != ns:
        raise PtcoreError("concerto_patch_pairs: one scene per selected row")
    e = ns * v
    empty = torch.empty(0, dtype=torch.int64, device=dev)
    if e == 0:
        return ConcertoPairs(empty, torch.zeros(1, dtype=torch.int64, device=dev), empty, torch.full((ns, v), -1, dtype=torch.int64, device=dev), rows)
    sentinel = max(int(total_images), 0) * int(patch_h) * int(patch_w)
    keys = torch.empty(e, dtype=torch.int64, device=dev)
    lib().ptc_concerto_pair_keys(ptr(corr.contiguous()), n, ptr(rows), ptr(scene.to(torch.int64).contiguous()),
                                 ptr(img_offset.to(torch.int64).contiguous()), ptr(img_num.to(torch.int64).contiguous()), ns,
                                 img_num.numel(), v, int(patch_h), int(patch_w), sentinel, ptr(keys), stream_ptr())
    order, _ = sort_keys(keys[None].contiguous(), 0, max(1, sentinel.bit_length()), want_inverse=False)
    order0 = order[0].contiguous()
    cluster = torch.empty(e, dtype=torch.int64, device=dev)
    ncl = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = lib().ptc_pool_maps_workspace_bytes(e)
    ws = _ws(nbytes, dev)
    lib().ptc_pool_maps_count(ptr(keys), ptr(order0), e, 0, ptr(cluster), ptr(ncl), ptr(ws), nbytes, stream_ptr())
    live = keys != sentinel
    n_cluster, n_pairs = torch.stack([ncl[0], live.sum()]).tolist()
    u = n_cluster - (1 if n_pairs < e else 0)          # the sentinel, where present, is the last run
    idx_ptr = torch.empty(n_cluster + 1, dtype=torch.int64, device=dev)
    head = torch.empty(n_cluster, dtype=torch.int64, device=dev)
    lib().ptc_pool_maps_fill(ptr(order0), ptr(cluster), e, n_cluster, ptr(idx_ptr), ptr(head), stream_ptr())
    point = torch.div(order0[:n_pairs], v, rounding_mode="floor")
    perm = point if rows is None else rows[point]
    pair_patch = torch.where(live, cluster, torch.full_like(cluster, -1)).view(ns, v)
    return ConcertoPairs(keys[head[:u]], idx_ptr[:u + 1].contiguous(), perm.contiguous(), pair_patch, rows)


def concerto_patch_mean_bwd(dmean: torch.Tensor, pairs: ConcertoPairs, n_out: int) -> torch.Tensor:
    """d feat3d [n_out, C] from d mean3d [U, C]: row p = sum over p's pairs of d mean3d[u] / count[u], gathered through
    pairs.pair_patch (no atomics); rows outside the selection are zero."""
    require_cuda(dmean)
    dmean = dmean.contiguous()
    u, c = dmean.shape
    ns, v = pairs.pair_patch.shape
    alloc = torch.empty if pairs.rows is None else torch.zeros
    out = alloc((int(n_out), c), dtype=dmean.dtype, device=dmean.device)
    lib().ptc_concerto_patch_mean_bwd(ptr(dmean), dtype_code(dmean), ptr(pairs.pair_patch.contiguous()), ptr(pairs.indptr), ptr(pairs.rows),
                                      ns, int(n_out), v, c, u, ptr(out), stream_ptr())
    return out


def concerto_align_supported(d: int) -> bool:
    """the centred-cosine kernel keeps a row in one wave's registers: up to 2048 channels"""
    return bool(lib().ptc_concerto_align_supported(int(d)))


def concerto_align(feature2d: torch.Tensor, patch_ids: torch.Tensor, y: torch.Tensor, cos_shift: bool, eps: float, want_dy: bool):
    """-> (loss [1] fp32 = 10 * mean_u (1 - cos(feature2d[patch_ids[u]], y[u])), row [U] fp32 = 1 - cos, dy [U, D] in y's dtype or
    None); with cos_shift both rows are centred over D first.  feature2d and y in fp32, bf16 or fp16 independently."""
    require_cuda(feature2d, patch_ids, y)
    ok = (torch.float32, torch.bfloat16, torch.float16)
    if feature2d.dim() != 2 or y.dim() != 2 or feature2d.shape[1] != y.shape[1] or feature2d.dtype not in ok or y.dtype not in ok:
        raise PtcoreError(f"concerto_align: feature2d {tuple(feature2d.shape)} {feature2d.dtype}, y {tuple(y.shape)} {y.dtype}")
    u, d = y.shape
    if patch_ids.numel() != u or u < 1 or not concerto_align_supported(d):
        raise PtcoreError(f"concerto_align: {patch_ids.numel()} ids for {u} rows (at least one) of {d} channels (at most 2048)")
    x, yy = feature2d.detach().contiguous(), y.detach().contiguous()
    ids = patch_ids.to(torch.int64).contiguous()
    row = torch.empty(u, dtype=torch.float32, device=y.device)
    loss = torch.empty(1, dtype=torch.float32, device=y.device)
    dy = torch.empty_like(yy) if want_dy else None
    lib().ptc_concerto_align(ptr(x), dtype_code(x), x.shape[0], ptr(ids), ptr(yy), dtype_code(yy), u, d, int(bool(cos_shift)), float(eps),
                             ptr(row), ptr(loss), ptr(dy), stream_ptr())
    return loss, row, dy


# ------------------------------------------------------------------------------------------------
# device-side point augmentation (csrc/augment.hip)
# ------------------------------------------------------------------------------------------------
# csrc/ptcore_augment.h: ptc_aug_compose descriptor kinds, ptc_aug_apply colour op kinds, and the per-call limits of both
AUG_CENTER_SHIFT, AUG_ROTATE, AUG_SCALE, AUG_FLIP, AUG_SHIFT = (_KA["PTC_AUG_" + k] for k in ("CENTER_SHIFT", "ROTATE", "SCALE", "FLIP", "SHIFT"))
AUG_C_AUTOCONTRAST, AUG_C_TRANSLATION, AUG_C_JITTER, AUG_C_NORMALIZE = (_KA["PTC_AUG_C_" + k] for k in ("AUTOCONTRAST", "TRANSLATION", "JITTER", "NORMALIZE"))
AUG_MAX_OPS, AUG_MAX_COLOR_OPS = _KA["PTC_AUG_MAX_OPS"], _KA["PTC_AUG_MAX_COLOR_OPS"]
AUG_STREAM_JITTER, AUG_STREAM_COLOR, AUG_STREAM_ELASTIC = 0, 1, 2                        # generator streams (elastic stage s: 2 + s)


def _aug_points(t: Optional[torch.Tensor], what: str, n: Optional[int] = None) -> Optional[torch.Tensor]:
    """[n, 3] fp32 contiguous (converted when it is anything else)"""
    if t is None:
        return None
    if t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
        raise PtcoreError(f"augment: {what} must be [{'n' if n is None else n}, 3], got {tuple(t.shape)}")
    if t.shape[0] == 0:
        raise PtcoreError("augment: empty point cloud")
    return t.to(torch.float32).contiguous()


def aug_state(device):
    """-> (aff [21] float64, stats [12] float64) on `device`, uninitialised: aug_compose(from_identity=True) / aug_reduce fill them"""
    return torch.empty(21, dtype=torch.float64, device=device), torch.empty(12, dtype=torch.float64, device=device)


def aug_reduce(coord: Optional[torch.Tensor], color: Optional[torch.Tensor], aff: Optional[torch.Tensor], stats: torch.Tensor) -> None:
    """stats[0:6] = min / max of A p + t over coord (aff None: of coord), stats[6:12] = channel min / max of color; a part given as None
    keeps its half.  One read-only pass and a finish launch; no host read."""
    require_cuda(coord, color, aff, stats)
    coord, color = _aug_points(coord, "coord"), _aug_points(color, "color")
    ref = coord if coord is not None else color
    if ref is None:
        raise PtcoreError("aug_reduce: neither coord nor color")
    n = ref.shape[0]
    partial = torch.empty((lib().ptc_aug_partials(n), 12), dtype=torch.float64, device=ref.device)
    lib().ptc_aug_reduce(ptr(coord), ptr(color), n, ptr(aff), ptr(partial), ptr(stats), stream_ptr())


def aug_compose(ops_list: Sequence[Sequence[float]], aff: torch.Tensor, stats: Optional[torch.Tensor], from_identity: bool) -> None:
    """advance the pending affine `aff` by the descriptors (kind, arguments...) in order; the ones that need the bounding box read it
    from `stats` on the device.  One launch per 16 descriptors; no host read."""
    require_cuda(aff, stats)
    ops_list = list(ops_list)
    if not ops_list and from_identity:
        ops_list = [(AUG_SHIFT, 0.0, 0.0, 0.0)]
    for at in range(0, len(ops_list), AUG_MAX_OPS):
        chunk = ops_list[at:at + AUG_MAX_OPS]
        flat = (ctypes.c_double * (8 * len(chunk)))()
        for i, op in enumerate(chunk):
            if len(op) > 8:
                raise PtcoreError(f"aug_compose: descriptor {op} has more than 8 entries")
            for j, v in enumerate(op):
                flat[i * 8 + j] = float(v)
        lib().ptc_aug_compose(ctypes.cast(flat, ctypes.c_void_p), len(chunk), int(bool(from_identity and at == 0)), ptr(aff), ptr(stats),
                              stream_ptr())


def aug_apply(coord=None, normal=None, color=None, aff=None, stats=None, jitter=None, clip_range=None, color_ops=(), want_stats=False):
    """The flush -> (coord', normal', color'), each None when its input is None; every given part is written once, into a new
    tensor.  jitter = (sigma, clip, noise [n,3] | None, seed); clip_range = six floats; color_ops = rows (kind, p0, p1, p2,
    noise [n,3] | None, seed, stream).  want_stats: stats[0:6] becomes the box of coord'.  No host read."""
    require_cuda(coord, normal, color, aff, stats)
    coord, normal, color = _aug_points(coord, "coord"), _aug_points(normal, "normal"), _aug_points(color, "color")
    ref = coord if coord is not None else normal if normal is not None else color
    if ref is None:
        raise PtcoreError("aug_apply: nothing to write")
    n, device = ref.shape[0], ref.device
    color_ops = list(color_ops)
    k = len(color_ops)
    flat = (ctypes.c_double * max(6 * k, 1))()
    noise_ptrs = (ctypes.c_void_p * max(k, 1))()
    keep = []
    for i, (kind, p0, p1, p2, noise, seed, stream) in enumerate(color_ops):
        noise = _aug_points(noise, "colour noise", n)
        require_cuda(noise)
        keep.append(noise)
        flat[i * 6:i * 6 + 6] = [float(kind), float(p0), float(p1), float(p2), float(int(seed) % (1 << 53)), float(stream)]
        noise_ptrs[i] = ptr(noise) or None
    jn = None
    if jitter is not None:
        jn = _aug_points(jitter[2], "jitter noise", n)
        require_cuda(jn)
    rng = None if clip_range is None else (ctypes.c_double * 6)(*[float(v) for v in clip_range])
    out_c = None if coord is None else torch.empty_like(coord)
    out_n = None if normal is None else torch.empty_like(normal)
    out_k = None if color is None else torch.empty_like(color)
    partial = torch.empty((lib().ptc_aug_partials(n), 6), dtype=torch.float64, device=device) if want_stats else None
    lib().ptc_aug_apply(ptr(coord), ptr(normal), ptr(color), n, ptr(aff), ptr(stats), int(jitter is not None),
                        float(jitter[0]) if jitter else 0.0, float(jitter[1]) if jitter else 1.0, ptr(jn),
                        int(jitter[3]) % (1 << 63) if jitter else 0, None if rng is None else ctypes.cast(rng, ctypes.c_void_p),
                        ctypes.cast(flat, ctypes.c_void_p), ctypes.cast(noise_ptrs, ctypes.c_void_p), k, ptr(out_c), ptr(out_n), ptr(out_k),
                        ptr(partial), ptr(stats) if want_stats else None, stream_ptr())
    return out_c, out_n, out_k


def aug_noise(seed: int, stream: int, count: int, device) -> torch.Tensor:
    """z [count] fp32: elements 0 .. count-1 of the generator's stream (seed, stream) -- what the kernels evaluate in place"""
    out = torch.empty(int(count), dtype=torch.float32, device=device)
    require_cuda(out)
    lib().ptc_aug_noise(int(seed) % (1 << 63), int(stream), int(count), ptr(out), stream_ptr())
    return out


def aug_elastic_grid(dims, noise: Optional[torch.Tensor], seed: int, stream: int, device) -> torch.Tensor:
    """-> grid [dx, dy, dz, 3] fp32: standard-normal noise (the given [dx, dy, dz, 3] tensor, or the generator's stream) after the
    reference's two rounds of width-3 box filters, in one launch"""
    dx, dy, dz = (int(d) for d in dims)
    if noise is not None:
        if tuple(noise.shape) != (dx, dy, dz, 3):
            raise PtcoreError(f"ElasticDistortion: noise of shape {tuple(noise.shape)} for a grid of {(dx, dy, dz, 3)}")
        buf = noise.to(device=device, dtype=torch.float32).contiguous()
    else:
        buf = torch.empty((dx, dy, dz, 3), dtype=torch.float32, device=device)
    grid = torch.empty((dx, dy, dz, 3), dtype=torch.float32, device=device)
    require_cuda(buf, grid)
    lib().ptc_aug_elastic_grid(ptr(buf), int(noise is None), int(seed) % (1 << 63), int(stream), dx, dy, dz, ptr(grid), stream_ptr())
    return grid


def aug_elastic_apply(coord: torch.Tensor, aff: Optional[torch.Tensor], stats: torch.Tensor, grid: torch.Tensor, granularity: float,
                      magnitude: float) -> torch.Tensor:
    """coord' [n,3] = p + trilinear(grid)(p) * magnitude with p = A coord + t; stats[0:3] = the min of p on entry, stats[0:6] = the box of
    coord' on return.  No host read."""
    require_cuda(coord, aff, stats, grid)
    coord = _aug_points(coord, "coord")
    n = coord.shape[0]
    dx, dy, dz = grid.shape[:3]
    out = torch.empty_like(coord)
    partial = torch.empty((lib().ptc_aug_partials(n), 6), dtype=torch.float64, device=coord.device)
    lib().ptc_aug_elastic_apply(ptr(coord), n, ptr(aff), ptr(stats), ptr(grid), dx, dy, dz, float(granularity), float(magnitude), ptr(out),
                                ptr(partial), ptr(stats), stream_ptr())
    return out
