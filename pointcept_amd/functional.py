"""Differentiable operators of the engine (torch.autograd.Function wrappers over pointcept_amd.ops).

Design rule: every backward is written in GATHER form over precomputed index maps, so no kernel
uses floating-point atomics and every result is bit-reproducible run to run:
  * backward of a row gather through a permutation-with-padding = a row gather through the inverse
    map (+ the duplicate slot),
  * backward of the unpooling gather = a segmented sum over the cluster CSR,
  * sparse-conv dgrad = the forward kernel on the transposed table / mirrored weights,
  * sparse-conv wgrad = per-split partial sums + a deterministic reduction.
"""
from __future__ import annotations

import math
import os
import weakref
from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, config, ops
from ._lib import PtcoreError


# ------------------------------------------------------------------------------------------------
# weight casts under autocast: ONE multi-tensor kernel per step instead of one cast kernel per layer
# ------------------------------------------------------------------------------------------------
# Every Linear / sparse-conv forward needs its fp32 master weight in the autocast dtype.  Casting at the
# point of use cost ~190 launches of 5 us per step (profiles/r01_k: bfloat16_copy_kernel).  The cache keeps
# one low-precision shadow per weight storage and, at the first miss after the optimizer step (version
# counters moved), refreshes ALL shadows with a single torch._foreach_copy_.
class _CastCache:
    """Entries die with the parameter they shadow (weak reference on the owning tensor: nothing here pins a discarded
    model's storage), are validated by the tensor's version counter, and can be dropped explicitly:
    `invalidate_weight_casts()` after writes that do not move the counter (`p.data.copy_()`, `p.data.mul_()` -- EMA /
    weight clipping code written against `.data`; optimizers, `load_state_dict` and `copy_` under `no_grad` do move it).
    A refresh between the forward and the backward of one live graph raises autograd's saved-tensor version error, as
    modifying the weight itself does in stock PyTorch."""

    def __init__(self, cuda_only: bool = True):
        self.entries = {}   # (data_ptr, numel, dtype) -> [weakref(owner), shadow (flat), version]
        self.cuda_only = cuda_only   # False only in the CPU unit test of this class
        # backward-pass layouts of the shadows ([c_in][taps][c_out], see layout()): shadow data_ptr -> entry, and
        # (shadow data_ptr, mode, taps_dst) -> [entry, buffer, shadow generation the buffer was made from, dims]
        self.by_shadow = {}
        self.layouts = {}
        self._desc = None   # (signature, desc tensor, prefix tensor, total)
        self._cast_desc = None   # the same for the one-launch cast (_cast_many)

    def invalidate(self) -> None:
        self._cast_desc = None
        self.entries.clear()
        self.by_shadow.clear()
        self.layouts.clear()
        self._desc = None

    _MODES = {"mirror": 0, "repeat": 1, "keep": 2}

    def layout(self, w: torch.Tensor, mode: str, taps_dst: int = 0) -> Optional[torch.Tensor]:
        """[c_in, taps', c_out] layout of a weight shadow for the input-gradient GEMMs: w = what get() returned, shape
        [c_out, c_in] or [c_out, taps, c_in]; mode "mirror" (taps reversed: submanifold dgrad; the plain transpose when
        taps = 1), "keep" (tap order kept) or "repeat" (taps = 1 matrix repeated taps_dst times).  Persistent buffers; every
        stale layout of the model is rewritten in ONE launch (ptc_weight_layouts) the first time one is asked for after the
        shadows were refreshed.  None when w is not a cache shadow (fp32 runs, padded copies): the caller permutes itself."""
        if not w.is_cuda or w.dim() not in (2, 3) or not w.is_contiguous() or w.element_size() != 2:
            return None
        e = self.by_shadow.get(w.data_ptr())
        if e is None or e[1].numel() != w.numel():
            return None
        co, ks, ci = (w.shape[0], 1, w.shape[1]) if w.dim() == 2 else tuple(w.shape)
        kd = int(taps_dst) if mode == "repeat" else ks
        if mode == "repeat" and ks != 1:
            return None
        key = (w.data_ptr(), mode, kd)
        lay = self.layouts.get(key)
        if lay is None:
            lay = self.layouts[key] = [e, torch.empty(ci * kd * co, dtype=w.dtype, device=w.device), None, (co, ks, ci, kd, self._MODES[mode])]
            self._desc = None
            self._refresh_layouts(w.device, only=key)      # first use: just this one (the table is rebuilt at the next full refresh)
        elif lay[2] != e[3]:
            self._refresh_layouts(w.device)
        return lay[1].view(ci, kd, co)

    def _refresh_layouts(self, device, only=None) -> None:
        live = [(k, v) for k, v in self.layouts.items() if v[0][0]() is not None and v[1].device == device and (only is None or k == only)]
        sig = tuple(k for k, _ in live)
        if only is not None or self._desc is None or self._desc[0] != sig:
            rows, prefix, total = [], [0], 0
            for _, (e, buf, _, (co, ks, ci, kd, mode)) in live:
                rows.append([e[1].data_ptr(), buf.data_ptr(), co, ks, ci, kd | (mode << 32)])
                total += ci * kd * co
                prefix.append(total)
            built = (sig, torch.tensor(rows, dtype=torch.int64, device=device), torch.tensor(prefix, dtype=torch.int64, device=device), total)
            if only is None:
                self._desc = built
        else:
            built = self._desc
        _, desc, prefix, total = built
        ops.weight_layouts(desc, prefix, len(live), total)
        for _, v in live:
            v[2] = v[0][3]

    def _cast_many(self, stale, srcs) -> bool:
        """ONE launch for the whole refresh (ptc_cast_many) instead of ~29 multi-tensor launches; False = not applicable."""
        if not stale or not all(s.is_cuda and s.dtype == torch.float32 for s in srcs):
            return False
        dts = {x[1].dtype for x in stale}
        if len(dts) != 1 or next(iter(dts)) not in (torch.bfloat16, torch.float16) or len({s.device for s in srcs}) != 1:
            return False
        sig = tuple((s.data_ptr(), x[1].data_ptr(), s.numel()) for x, s in zip(stale, srcs))
        dt = next(iter(dts))
        if self._cast_desc is None:
            self._cast_desc = {}
        if dt not in self._cast_desc or self._cast_desc[dt][0] != sig:
            rows, prefix, units = [], [0], 0
            for src_ptr, dst_ptr, numel in sig:
                rows.append([src_ptr, dst_ptr, numel])
                units += (numel + 7) // 8
                prefix.append(units)
            dev = srcs[0].device
            self._cast_desc[dt] = (sig, torch.tensor(rows, dtype=torch.int64, device=dev), torch.tensor(prefix, dtype=torch.int64, device=dev), units)
        _, desc, prefix, units = self._cast_desc[dt]
        ops.cast_many(desc, prefix, len(sig), units, dt)
        return True

    def get(self, w: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
        if w.dtype == dt:
            return w
        owner = w._base if w._base is not None else w     # conv weights arrive as views of the Parameter
        if not isinstance(owner, torch.nn.Parameter) and (owner.grad_fn is not None or not owner.is_leaf):   # a weight COMPUTED this step: nothing to cache
            return w.to(dt)
        if not w.is_contiguous() or (self.cuda_only and not w.is_cuda) or owner.numel() != w.numel() or not owner.is_contiguous():
            return w.to(dt)
        key = (w.data_ptr(), w.numel(), dt)
        e = self.entries.get(key)
        if e is not None and e[0]() is not owner:          # address reused by another tensor
            e = None
        if e is not None and e[2] == owner._version:
            return e[1].view(w.shape)
        if e is None:
            entries = self.entries

            def _drop(_ref, key=key, entries=entries, cache=self):
                cur = entries.get(key)
                if cur is not None and cur[0] is _ref:
                    del entries[key]
                    ptr = cur[1].data_ptr()
                    cache.by_shadow.pop(ptr, None)
                    for k in [k for k in cache.layouts if k[0] == ptr]:
                        del cache.layouts[k]
                    cache._desc = None

            e = [weakref.ref(owner, _drop), torch.empty(w.numel(), dtype=dt, device=w.device), -1, 0]   # ..., generation of the shadow
            self.entries[key] = e
            self.by_shadow[e[1].data_ptr()] = e
        # one multi-tensor copy refreshes every stale shadow (the first miss after an optimizer step)
        stale, srcs = [], []
        for x in list(self.entries.values()):
            o = x[0]()
            if o is not None and x[2] != o._version:
                stale.append(x)
                srcs.append(o.detach().reshape(-1))
        # per shadow dtype: a process that ran bf16 AND fp16 autocast holds both kinds, and torch._foreach_copy_ on a destination list
        # of mixed dtypes converts every tensor to the FIRST one's dtype on the CUDA fast path (seen on PyTorch 2.10 / ROCm 7: the
        # second dtype's shadows received the first dtype's bit patterns -- tools/fp16_stem_probe.py)
        with torch.no_grad():
            for dt_ in {x[1].dtype for x in stale}:
                grp = [(x, s_) for x, s_ in zip(stale, srcs) if x[1].dtype == dt_]
                gx, gs = [g_[0] for g_ in grp], [g_[1] for g_ in grp]
                if not self._cast_many(gx, gs):
                    torch._foreach_copy_([x[1] for x in gx], gs)
        for x, o in zip(stale, srcs):
            x[2] = x[0]()._version
            x[3] += 1
        return e[1].view(w.shape)


# The per-step refresh of the 16-bit weight shadows is ONE launch (csrc/rows.hip: cast_many_kernel; _CastCache._cast_many) where every
# stale shadow is a CUDA fp32 -> bf16 / f16 pair on one device, torch._foreach_copy_ (~29 multi-tensor launches at the bench config) otherwise.
# Timed in the step: 49.4 vs 49.8 ms (profiles/r03_a_knob_ab.txt) -- neutral on the GPU clock, 28 launches less on the host.
_cast_cache = _CastCache()


def invalidate_weight_casts() -> None:
    """Drop every low-precision weight shadow (call after `.data` writes to parameters, see _CastCache)."""
    _cast_cache.invalidate()


def _autocast_on() -> bool:
    return torch.is_autocast_enabled("cuda")


def _autocast_dtype(t: torch.Tensor) -> torch.dtype:
    if _autocast_on():
        return torch.get_autocast_dtype("cuda")
    return t.dtype


# ------------------------------------------------------------------------------------------------
# row gathers
# ------------------------------------------------------------------------------------------------
class _GatherRows(Function):
    @staticmethod
    def forward(ctx, src, idx, bwd_idx, bwd_idx2):
        ctx.save_for_backward(bwd_idx, bwd_idx2)
        return ops.gather_rows(src, idx)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        bwd_idx, bwd_idx2 = ctx.saved_tensors
        return ops.gather_rows(grad.contiguous(), bwd_idx, bwd_idx2), None, None, None


def gather_rows(src: torch.Tensor, idx: torch.Tensor, bwd_idx: torch.Tensor,
                bwd_idx2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = src[idx[i]].  `bwd_idx` [n_src] (and optional `bwd_idx2`) list, for every source row,
    the output row(s) it was copied to (-1 = none): grad_src[p] = g[bwd_idx[p]] + g[bwd_idx2[p]]."""
    return _GatherRows.apply(src, idx, bwd_idx, bwd_idx2)


class _GatherByCluster(Function):
    @staticmethod
    def forward(ctx, src, cluster, perm, indptr):
        ctx.save_for_backward(perm, indptr)
        return ops.gather_rows(src, cluster)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        perm, indptr = ctx.saved_tensors
        gsrc, _ = ops.segment_csr_fwd(grad.contiguous(), perm, indptr, "sum")
        return gsrc, None, None, None


class _GatherByClusterAdd(Function):
    """addend + src[cluster] in one kernel; the gradient of the addend is the incoming gradient itself"""

    @staticmethod
    def forward(ctx, src, cluster, perm, indptr, addend):
        ctx.save_for_backward(perm, indptr)
        return ops.gather_rows_add(src, cluster, addend)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        perm, indptr = ctx.saved_tensors
        grad = grad.contiguous()
        gsrc, _ = ops.segment_csr_fwd(grad, perm, indptr, "sum")
        return gsrc, None, None, None, grad


def gather_by_cluster_add(addend: torch.Tensor, src: torch.Tensor, cluster: torch.Tensor, perm: torch.Tensor, indptr: torch.Tensor):
    """addend + src[cluster] (SerializedUnpooling, ptv3m1:478: `parent.feat + point.feat[inverse]`) -- one pass where the kernel serves the
    shape (same 16-bit / fp32 dtype on both sides, rows of whole 16-byte lanes), the gather followed by torch's add otherwise."""
    if ops.gather_rows_add_supported(src, addend) and addend.shape[0] == cluster.numel():
        return _GatherByClusterAdd.apply(src, cluster, perm, indptr, addend)
    return addend + gather_by_cluster(src, cluster, perm, indptr)


def gather_by_cluster(src: torch.Tensor, cluster: torch.Tensor, perm: torch.Tensor, indptr: torch.Tensor):
    """out[p] = src[cluster[p]] (SerializedUnpooling, ptv3m1:478).  Backward = segmented sum over
    the cluster CSR (perm = points sorted by cluster, indptr = idx_ptr)."""
    return _GatherByCluster.apply(src, cluster, perm, indptr)


# ------------------------------------------------------------------------------------------------
# segment_csr
# ------------------------------------------------------------------------------------------------
class _SegmentCSR(Function):
    @staticmethod
    def forward(ctx, src, perm, indptr, reduce, covers_all):
        out, arg = ops.segment_csr_fwd(src, perm, indptr, reduce)
        ctx.reduce = reduce
        ctx.covers_all = covers_all
        ctx.n_src = src.shape[0]
        ctx.save_for_backward(perm, indptr, arg)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        perm, indptr, arg = ctx.saved_tensors
        g = ops.segment_csr_bwd(grad.contiguous(), perm, indptr, arg, ctx.n_src, ctx.reduce, ctx.covers_all)
        return g, None, None, None, None


def segment_csr(src: torch.Tensor, indptr: torch.Tensor, reduce: str = "sum", perm: Optional[torch.Tensor] = None,
                covers_all: bool = False):
    """torch_scatter.segment_csr(src[perm], indptr, reduce) with the gather fused (ptv3m1:416-421).
    covers_all: the caller guarantees that the segments partition ALL rows of src (indptr[0] = 0, indptr[-1] = N, perm a
    permutation -- the pooling layers build them that way): the backward then writes every row and skips the zero fill."""
    if src.dim() == 1:
        return _SegmentCSR.apply(src[:, None], perm, indptr, reduce, covers_all)[:, 0]
    return _SegmentCSR.apply(src, perm, indptr, reduce, covers_all)


# ------------------------------------------------------------------------------------------------
# sparse convolution
# ------------------------------------------------------------------------------------------------
def _pad_to(x: torch.Tensor, dim: int, mult: int) -> torch.Tensor:
    c = x.shape[dim]
    r = (-c) % mult
    if r == 0:
        return x
    pad = [0, 0] * (x.dim() - 1 - dim) + [0, r]
    return F.pad(x, pad)


# The duplicate merge is ONE segmented sum (ptc_segment_csr_fwd) over a CSR of the representatives that is built once per coordinate
# set -- no python loop, no host sync per conv backward; additions in ascending row order.
_dup_csr = {}   # id(rep) -> (weakref(rep), perm, indptr, keep)


def _dup_csr_of(rep: torch.Tensor):
    e = _dup_csr.get(id(rep))
    if e is not None and e[0]() is rep:
        return e[1:]
    n = rep.shape[0]
    perm = torch.sort(rep, stable=True).indices                       # rows grouped by representative, ascending row inside a group
    counts = torch.bincount(rep, minlength=n)
    indptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
    keep = counts == 0                                                # rows that are copies: nothing is summed INTO them
    key = id(rep)

    def _drop(ref, key=key):
        cur = _dup_csr.get(key)
        if cur is not None and cur[0] is ref:
            del _dup_csr[key]

    _dup_csr[key] = (weakref.ref(rep, _drop), perm, indptr, keep)
    return perm, indptr, keep


def _merge_duplicate_rows(g: torch.Tensor, rep: torch.Tensor) -> torch.Tensor:
    """g with, for every voxel listed more than once, the rows of all its copies summed into the representative row
    rep[i] (the lowest row of the voxel).  Only runs for inputs that carry duplicate coordinates (Mix3D batches); no atomics, fixed order."""
    perm, indptr, keep = _dup_csr_of(rep)
    merged, _ = ops.segment_csr_fwd(g.contiguous(), perm, indptr, "sum")   # row t: g[t] + its copies, ascending rows
    return torch.where(keep[:, None], g, merged.to(g.dtype))


_rev_index_cache = {}
def _reverse_index(n: int, device) -> torch.Tensor:
    key = (n, device)
    t = _rev_index_cache.get(key)
    if t is None:
        t = _rev_index_cache[key] = torch.arange(n - 1, -1, -1, device=device)
    return t


# (Weight gradients on a second HIP stream beside the input gradient were measured SLOWER in the step -- 52.6-53.6 against 51.1-51.8 ms,
#  profiles/r02_t_bench_ab.txt: two cross-stream waits per Function cost more than the small kernels gain -- and removed.)


# ---- cast twins of activations --------------------------------------------------------------------
# The fused residual joint writes the fp32 stream x AND its autocast-dtype copy in one pass (add_norm: y = cast(z)).  GEMM
# wrappers that would cast x again (pooling / unpooling projections, the segmentation head: 13 casts of [N, C] per step at
# the bench config, and 13 more in the backward) look the copy up here instead.  Same values (one RNE rounding of the same
# fp32 number); the gradient then reaches the joint through its `y` output, which the kernel adds in fp32.
_act_twins = {}   # id(x) -> (weakref(x), twin, x._version)


def register_cast_twin(x: torch.Tensor, twin: torch.Tensor) -> None:
    key = id(x)

    def _drop(ref, key=key):
        cur = _act_twins.get(key)
        if cur is not None and cur[0] is ref:
            del _act_twins[key]

    _act_twins[key] = (weakref.ref(x, _drop), twin, x._version)


def cast_twin(x: torch.Tensor, dt: torch.dtype) -> Optional[torch.Tensor]:
    e = _act_twins.get(id(x))
    if e is not None and e[0]() is x and e[2] == x._version and e[1].dtype == dt and e[1].shape == x.shape:
        return e[1]
    return None


class _SparseConv(Function):
    """out = conv(feat; weight [C_out, kv, C_in], bias) over gather table `nbr`;
    `nbr_t` is the table of the transposed map (SubM: the same table, with mirrored weights).

    Duplicate voxel coordinates (legal input: Mix3D) make the maps many-to-one -- every copy of a voxel reads
    the SAME neighbour rows (lowest row wins in the hash) and no row ever reads a non-lowest copy -- so the transposed
    gather needs two corrections to stay the exact adjoint: `dup_out` = representative row of every OUTPUT row (the
    incoming gradient of the copies is first summed into their representative), `dup_in` = representative row of every
    INPUT row (copies that nothing reads get a zero gradient).  Both None for duplicate-free coordinates."""

    @staticmethod
    def forward(ctx, feat, weight, bias, nbr, nbr_t, mirror, dup_out, dup_in, blocks):
        dt = _autocast_dtype(feat)
        c_out, kv, c_in = weight.shape
        # channels are padded to 16; a stem (c_in <= 8: 6 colour + normal channels, k = 5) only to 8: its gathered rows are then 16
        # bytes and conv3 packs four table rows into one MFMA step (csrc/conv3.h, KPC = 16)
        cpad = 8 if (c_in <= 8 and kv > 1 and dt != torch.float32) else 16
        opad = 16
        if (blocks is not None and kv == 27 and c_in == c_out and 16 < c_in < 64 and c_in != 32 and dt != torch.float32
                and ops.block_plan(64, 64, 27, dt, feat.shape[0]) is not None):
            # round 5: a square submanifold 3^3 convolution of 17 .. 63 channels (PT-v3m2's 48, LitePT's 36 at stage 0) on the block-staged,
            # register-weight kernels of the next width they exist for (conv7 / wgrad7: 32 | 64 channels), zero-padded: the 48-channel
            # stage-0 convolutions ran 403 us on conv2 against 145 us for conv7 at 64 (profiles/r05_m_m2_kernel_stats.csv)
            cpad = opad = 32 if c_in < 32 else 64
        # (measured and dropped, round 5: SpUNet's 96-channel level-0 convolutions zero-padded onto the 128-channel instances -- step 26.7 -> 31.2 ms)
        f = _pad_to(feat.to(dt), 1, cpad).contiguous()
        w = _pad_to(_pad_to(_cast_cache.get(weight, dt), 2, cpad), 0, opad).contiguous()
        b = None if bias is None else _pad_to(bias.float(), 0, opad)
        # (padding the 6 -> 16 channel stem further to 32 so that conv3 takes it was measured SLOWER than conv2:
        #  1.20 ms vs 0.74 ms for the 125-offset table, r01_u)
        # blocks = ops.BlockProvider of the (submanifold) table: the LDS-staged kernel where the shape allows it
        blk = None if blocks is None else blocks.get(f.shape[1], w.shape[0], dt, conv=True)
        out = ops.spconv_fwd(f, w, b, nbr, blk)
        ctx.save_for_backward(f, w, nbr, nbr_t, dup_out, dup_in)
        ctx.blocks = blocks if mirror else None    # SubM: dgrad runs over the same table
        ctx.mirror = mirror
        ctx.shape = (c_out, kv, c_in)
        ctx.in_dtype, ctx.w_dtype = feat.dtype, weight.dtype
        ctx.has_bias = bias is not None
        return out[:, :c_out] if out.shape[1] != c_out else out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        f, w, nbr, nbr_t, dup_out, dup_in = ctx.saved_tensors
        c_out, kv, c_in = ctx.shape
        g = _pad_to(grad.to(f.dtype), 1, w.shape[0] if w.shape[0] == f.shape[1] and w.shape[0] in (32, 64) else 16).contiguous()
        dfeat = dw = dbias = None
        if ctx.needs_input_grad[1]:
            # submanifold 3^3, 32 | 64 channels: the block-staged weight gradient over the tables the forward built (csrc/wgrad7.h)
            blkw = None if (ctx.blocks is None or not config.WGRAD_BLK) else ctx.blocks.get(f.shape[1], g.shape[1], f.dtype)
            dw = ops.spconv_wgrad(f, g, nbr, blk=blkw)[:c_out, :, :c_in].to(ctx.w_dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            dbias = ops.column_sum(grad)
        if ctx.needs_input_grad[0]:
            wt = _cast_cache.layout(w, "mirror" if ctx.mirror else "keep")   # all layers' layouts in one launch per step
            if wt is None:
                wt = w.permute(2, 1, 0)
                if ctx.mirror:   # W' = W.permute(ci, k, co).flip(k), contiguous, in ONE launch (flip + contiguous were two)
                    wt = wt.index_select(1, _reverse_index(wt.shape[1], wt.device))
                else:
                    wt = wt.contiguous()
            gm = g if dup_out is None else _merge_duplicate_rows(g, dup_out)
            blk = None if ctx.blocks is None else ctx.blocks.get(gm.shape[1], wt.shape[0], gm.dtype, conv=True)
            dfeat = ops.spconv_fwd(gm, wt, None, nbr_t, blk)[:, :c_in].to(ctx.in_dtype)
            if dup_in is not None:
                own = dup_in == torch.arange(dup_in.numel(), device=dup_in.device, dtype=dup_in.dtype)
                dfeat = dfeat * own[:, None].to(dfeat.dtype)
        return dfeat, dw, dbias, None, None, None, None, None, None


def sparse_conv(feat, weight, bias, nbr, nbr_t, mirror: bool, dup_out=None, dup_in=None, blocks=None):
    """weight: [C_out, kv, C_in] (a view of the spconv-layout parameter [C_out,k0,k1,k2,C_in]).  blocks: optional
    ops.BlockProvider of `nbr` (submanifold tables only)."""
    return _SparseConv.apply(feat, weight, bias, nbr, nbr_t, mirror, dup_out, dup_in, blocks)


# ------------------------------------------------------------------------------------------------
# dense row-wise GEMM (nn.Linear on [N,C] point features) on the sparse-conv MFMA kernels
# ------------------------------------------------------------------------------------------------
# Shape policy: contractions of <= 256 channels run on the persistent linear2 kernel, wider ones on the chunked implicit-GEMM kernel with
# an identity table (csrc/conv3.h, IDENT: multiples of 128 -- PTv3's fc2 / dgrad-of-fc1 / qkv / proj of the 128..512-channel stages --
# and, round 5, every multiple of 32 through its general chunking: the 288 .. 2304-wide MLPs of PT-v3m2 / m3 / LitePT), every weight
# gradient on the split-K kernel (wgrad2).  Operands are zero-padded to the kernels' granularity (`_gemm_pad`): 16 channels, 32 on
# both sides as soon as either side of the GEMM exceeds 256 (its input-gradient GEMM contracts over the OUTPUT width).  There is no
# library GEMM behind this file (rounds 2-4 sent what the kernels did not cover to hipBLASLt).
def _own_gemm(n_rows: int, k: int, dtype: torch.dtype, c_out: int = 32) -> bool:
    return dtype != torch.float32 and (k <= 256 or (k % 32 == 0 and c_out % 32 == 0))


def _gemm_pad(c_in: int, c_out: int, dtype: torch.dtype) -> int:
    return 32 if (dtype != torch.float32 and (c_in > 256 or c_out > 256)) else 16


class _Linear(Function):
    """out[o] = W x[tab[o]] + b.  tab_fwd [1, n_out] int32 (None = identity) folds a row gather into
    the GEMM; tab_bwd [k, n_in] int32 lists, for every input row, the output rows that read it
    (-1 = none), which makes the input gradient a gather too: dx[p] = sum_k dout[tab_bwd[k][p]] W."""

    @staticmethod
    def forward(ctx, x, weight, bias, tab_fwd, tab_bwd):
        dt = _autocast_dtype(x)
        c_out, c_in = weight.shape
        pad = _gemm_pad(c_in, c_out, dt)
        xp = _pad_to(x.to(dt), 1, pad).contiguous()
        wp = _pad_to(_pad_to(_cast_cache.get(weight, dt), 1, pad), 0, pad).contiguous()
        bp = None if bias is None else _pad_to(bias.float(), 0, pad)
        out = ops.spconv_fwd(xp, wp[:, None, :], bp, tab_fwd)        # linear2 / conv3 (identity table) / the fp32 kernels: no library GEMM
        ctx.pad = pad
        ctx.save_for_backward(xp, wp, tab_fwd, tab_bwd)
        ctx.shape = (c_out, c_in)
        ctx.in_dtype, ctx.w_dtype = x.dtype, weight.dtype
        ctx.b_dtype = None if bias is None else bias.dtype
        return out[:, :c_out] if out.shape[1] != c_out else out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        xp, wp, tab_fwd, tab_bwd = ctx.saved_tensors
        c_out, c_in = ctx.shape
        g = _pad_to(grad.to(xp.dtype), 1, ctx.pad).contiguous()
        dx = dw = db = None
        want_b = ctx.b_dtype is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            res = ops.spconv_wgrad(xp, g, tab_fwd, want_bias=want_b)
            dwp, dbp = res if want_b else (res, None)
            dw = dwp[:c_out, 0, :c_in].to(ctx.w_dtype)
            if want_b:
                db = dbp[:c_out].to(ctx.b_dtype)
        if ctx.needs_input_grad[0]:
            slots = tab_bwd.shape[0] if tab_bwd is not None else 1
            wt = _cast_cache.layout(wp, "repeat", slots) if slots > 1 else _cast_cache.layout(wp, "mirror")
            if wt is None:
                wt = wp.t().contiguous()[:, None, :]                       # [c_in, 1, c_out]
                if slots > 1:
                    wt = wt.expand(-1, slots, -1).contiguous()              # same W for every slot
            dx = ops.spconv_fwd(g, wt, None, tab_bwd)
            dx = dx[:, :c_in].to(ctx.in_dtype)
        return dx, dw, db, None, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
           tab_fwd: Optional[torch.Tensor] = None, tab_bwd: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.linear for [N, C_in] point features: out = x W^T + b, autocast-aware (bf16 operands, fp32
    accumulate), forward / dgrad / wgrad (+ fused bias gradient) on the identity-table MFMA kernels.
    With (tab_fwd, tab_bwd) the GEMM also applies a row permutation-with-padding:
    out[o] = W x[tab_fwd[0][o]] + b  (= F.linear(x)[tab] = F.linear(x[tab]): a row-wise map commutes
    with a row gather), which removes the separate gather pass around serialized attention."""
    if x.dim() != 2:
        raise PtcoreError("linear expects [N, C] features")
    if (tab_fwd is None) != (tab_bwd is None):
        raise PtcoreError("linear: tab_fwd and tab_bwd go together")
    return _Linear.apply(x, weight, bias, tab_fwd, tab_bwd)


# ------------------------------------------------------------------------------------------------
# layer norm
# ------------------------------------------------------------------------------------------------
class _LayerNorm(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_dtype):
        y, mean, rstd = ops.layer_norm_fwd(x, weight, bias, eps, out_dtype)
        ctx.save_for_backward(x, mean, rstd, weight)
        ctx.has_affine = weight is not None
        ctx.has_bias = bias is not None          # nn.LayerNorm(bias=False): no gradient may be returned for the absent input
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, mean, rstd, weight = ctx.saved_tensors
        dx, dg, db = ops.layer_norm_bwd(dy, x, mean, rstd, weight, want_affine=ctx.has_affine)
        if ctx.has_affine:
            dg, db = dg.to(weight.dtype), (db.to(weight.dtype) if ctx.has_bias else None)
        return dx, dg, db, None, None


def layer_norm(x: torch.Tensor, weight, bias, eps: float = 1e-5, out_dtype: Optional[torch.dtype] = None):
    """nn.LayerNorm over the last dim of [N,C].  Default output dtype follows PyTorch: fp32 under
    autocast (layer_norm is an fp32 autocast op) else x.dtype; `out_dtype=torch.bfloat16` lets the
    caller take the value already rounded for a following bf16 GEMM (same number the autocast
    cast would produce, one HBM pass less)."""
    if out_dtype is None:
        out_dtype = torch.float32 if (_autocast_on() or x.dtype == torch.float32) else x.dtype
    return _LayerNorm.apply(x, weight, bias, float(eps), out_dtype)


# ------------------------------------------------------------------------------------------------
# fused residual joint: z = a + row_scale * LN_A(u),  y = LN_B(z)
# ------------------------------------------------------------------------------------------------
class _AddNorm(Function):
    @staticmethod
    def forward(ctx, u, a, row_scale, ga, ba, eps_a, gb, bb, eps_b, has_a, has_b, y_dtype):
        norm_a = (None if ga is None else ga.float(), None if ba is None else ba.float(), eps_a) if has_a else None
        norm_b = (None if gb is None else gb.float(), None if bb is None else bb.float(), eps_b) if has_b else None
        z, y, st_a, st_b = ops.add_norm_fwd(u, a, row_scale, norm_a, norm_b, y_dtype)
        ctx.save_for_backward(u, z, row_scale, st_a, st_b, None if norm_a is None else norm_a[0],
                              None if norm_b is None else norm_b[0])
        ctx.has_a, ctx.has_b = has_a, has_b
        ctx.aff = (ga is not None, gb is not None)
        ctx.has_bias = (ba is not None, bb is not None)     # a weight-only LayerNorm gets no bias gradient back (autograd raises on one)
        ctx.a_dtype = a.dtype
        # an unused output (the cast copy of a stage's last block, which the pooling does not read) must not be
        # materialised as a zero gradient: that was 8 zero fills + 8 extra reads of [N, C] per step
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable()
        if y is None:
            y = z.new_empty(0)
            ctx.mark_non_differentiable(y)
        return z, y

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, dy):
        u, z, row_scale, st_a, st_b, ga, gb = ctx.saved_tensors
        if dy is not None and dy.numel() == 0:
            dy = None
        if dz is None and dy is None:
            return (None,) * 12
        da, du, dga, dba, dgb, dbb = ops.add_norm_bwd(dz, dy, z, u, row_scale, ga, st_a, gb, st_b,
                                                      ctx.has_a and ctx.aff[0], ctx.has_b and ctx.aff[1] and dy is not None,
                                                      da_dtype=ctx.a_dtype)
        return du, da, None, dga, (dba if ctx.has_bias[0] else None), None, dgb, (dbb if ctx.has_bias[1] else None), None, None, None, None


def add_norm(u: torch.Tensor, a: torch.Tensor, row_scale: Optional[torch.Tensor] = None, norm_a=None, norm_b=None,
             y_dtype: Optional[torch.dtype] = None):
    """One pass over a residual joint of the PTv3 Block: z = a + row_scale[:,None] * f(u) (fp32 residual
    stream), y = g(z) as `y_dtype`.  f / g are nn.LayerNorm modules (norm_a / norm_b) or identity.
    Returns (z, y); y is None when y_dtype is None."""
    if a.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        a = a.float()
    ga, ba, ea = (norm_a.weight, norm_a.bias, norm_a.eps) if norm_a is not None else (None, None, 0.0)
    gb, bb, eb = (norm_b.weight, norm_b.bias, norm_b.eps) if norm_b is not None else (None, None, 0.0)
    z, y = _AddNorm.apply(u, a, row_scale, ga, ba, float(ea), gb, bb, float(eb), norm_a is not None, norm_b is not None,
                          y_dtype)
    return z, (y if y_dtype is not None else None)


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
class _AttnVarlen(Function):
    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, softmax_scale, dropout_p, seed):
        out, lse = ops.attn_varlen_fwd(qkv, cu_seqlens, max_seqlen, softmax_scale, dropout_p, seed)
        ctx.save_for_backward(qkv, out, lse, cu_seqlens)
        ctx.max_seqlen, ctx.scale, ctx.drop = max_seqlen, softmax_scale, (dropout_p, seed)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, out, lse, cu = ctx.saved_tensors
        dqkv = ops.attn_varlen_bwd(qkv, out, dout.contiguous(), lse, cu, ctx.max_seqlen, ctx.scale, *ctx.drop)
        return dqkv, None, None, None, None, None


def attn_varlen_qkvpacked(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int,
                          softmax_scale: Optional[float] = None, dropout_p: float = 0.0, seed: Optional[int] = None) -> torch.Tensor:
    """flash_attn.flash_attn_varlen_qkvpacked_func semantics (ptv3m1:208-214),
    non-causal, qkv [T,3,H,16] bf16 -> [T,H,16] bf16.  f16 qkv with head_dim 16 = the reference's fp16-autocast call site INCLUDING its
    casts: `flash_attn(qkv.to(bfloat16)).to(qkv.dtype)` -- bf16 arithmetic, f16 tensors, the four cast passes (two forward, two
    backward) folded into the kernels' loads and stores; f16 qkv with head_dim 17..64 = f16 OPERANDS (f16 MFMAs, f16 P / dS, fp32
    accumulation: what flash-attn does with LitePT's fp16 tensors, litept_v1.py:259-265).  dropout_p > 0 (head_dim 16): attention dropout; the mask is a function of
    `seed` (default: drawn from torch's CPU generator, so torch.manual_seed reproduces a step) and is regenerated by the backward."""
    if qkv.dtype not in (torch.bfloat16, torch.float16):
        raise PtcoreError("attn_varlen_qkvpacked expects 16-bit operands (the reference casts with .to(torch.bfloat16), ptv3m1:209)")
    if softmax_scale is None:
        softmax_scale = qkv.shape[-1] ** -0.5
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:
        raise PtcoreError("dropout_p must lie in [0, 1)")
    if dropout_p > 0.0 and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())        # CPU generator: no device synchronisation
    return _AttnVarlen.apply(qkv, cu_seqlens, int(max_seqlen), float(softmax_scale), dropout_p, int(seed or 0))


class _AttnRpe(Function):
    @staticmethod
    def forward(ctx, qkv, rpe_table, cu_seqlens, grid_coord, max_seqlen, softmax_scale, pos_bnd):
        out, lse = ops.attn_rpe_fwd(qkv, cu_seqlens, max_seqlen, softmax_scale, grid_coord, rpe_table.float(), pos_bnd)
        ctx.save_for_backward(qkv, out, lse, cu_seqlens, grid_coord, rpe_table)
        ctx.args = (max_seqlen, softmax_scale, pos_bnd)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, out, lse, cu, gc, tab = ctx.saved_tensors
        max_seqlen, scale, pos_bnd = ctx.args
        dqkv, dtab = ops.attn_rpe_bwd(qkv, out, dout.contiguous(), lse, cu, max_seqlen, scale, gc, tab.float(), pos_bnd)
        return dqkv, dtab.to(tab.dtype), None, None, None, None, None


def attn_rpe_qkvpacked(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int, softmax_scale: float,
                       grid_coord: torch.Tensor, rpe_table: torch.Tensor, pos_bnd: int) -> torch.Tensor:
    """The reference's dense attention branch with RPE (ptv3m1:29-48,190-206) on the window-attention kernels:
    softmax(scale q k^T + rpe(grid_coord_i - grid_coord_j)) v per window, qkv [T,3,H,16] bf16 or f16 (bf16 operands, fp32
    softmax) or fp32 (fp32 throughout) in serialized order, grid_coord [T,3] int32 in the same order, rpe_table [3(2B+1), H]
    (differentiable)."""
    if qkv.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise PtcoreError("attn_rpe_qkvpacked expects bf16, f16 or fp32 qkv")
    return _AttnRpe.apply(qkv, rpe_table, cu_seqlens, grid_coord, int(max_seqlen), float(softmax_scale), int(pos_bnd))


# ------------------------------------------------------------------------------------------------
# PT-v3m3 Point3DRoPE on packed qkv rows
# ------------------------------------------------------------------------------------------------
class _RopeXYZ(Function):
    """ptc_rope3d_xyz: q / k slabs rotated, v converted, one pass, bf16 out; backward = the inverse rotation of the gradient."""

    @staticmethod
    def forward(ctx, qkv, xyz, inv_freq, out_dtype):
        ctx.save_for_backward(xyz, inv_freq)
        ctx.in_dtype = qkv.dtype
        return ops.rope3d_xyz(qkv.contiguous(), xyz, inv_freq, 2, 1.0, out_dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xyz, inv_freq = ctx.saved_tensors
        return ops.rope3d_xyz(g.contiguous(), xyz, inv_freq, 2, -1.0, ctx.in_dtype), None, None, None


def rope_xyz_torch(qkv: torch.Tensor, xyz: torch.Tensor, inv_freq: torch.Tensor) -> torch.Tensor:
    """The reference's arithmetic (point_transformer_v3m3_utonia.py:58-101,303-323) on the packed layout, in torch ops:
    qkv [n, 3, H, D] of any float dtype -> bf16; q and k are rotated in fp32 (bf16 * fp32 promotes there too), v is only cast."""
    n, _, H, D = qkv.shape
    Q = D // 6
    emb = xyz[:, :, None] * inv_freq[None, None, :]                       # [n, 3, Q]   (:62-67)
    cos, sin = emb.cos()[:, None, None, :, None, :], emb.sin()[:, None, None, :, None, :]   # over (slab, head, axis, half, i)
    t = qkv[:, :2].float().reshape(n, 2, H, 3, 2, Q)
    u, v = t[..., 0:1, :], t[..., 1:2, :]
    rot = torch.cat((u * cos + (-v) * sin, v * cos + u * sin), dim=-2)     # x cos + rotate_half(x) sin  (:75-77,91-92)
    return torch.cat((rot.reshape(n, 2, H, D).to(torch.bfloat16), qkv[:, 2:].to(torch.bfloat16)), dim=1)


def rope_xyz_qkvpacked(qkv: torch.Tensor, xyz: torch.Tensor, inv_freq: torch.Tensor, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """qkv [n, 3, H, D] (D % 6 == 0) -> bf16 [n, 3, H, D] with Point3DRoPE applied to q and k: what flash-attn receives at
    point_transformer_v3m3_utonia.py:319-323.  On ptc_rope3d_xyz (one pass over the packed rows, bf16 out); `rope_xyz_torch` is the same
    arithmetic in torch ops, kept as the reference of the parity tests."""
    if qkv.dim() != 4 or qkv.shape[1] != 3 or qkv.shape[3] % 6 != 0:
        raise PtcoreError(f"rope_xyz_qkvpacked: qkv {tuple(qkv.shape)} must be [n, 3, H, D] with D % 6 == 0")
    # out_dtype: bf16 = PT-v3m3's `qkv.to(torch.bfloat16)` in front of flash-attn; LitePT hands over its autocast dtype (f16 under the fp16 recipe)
    return _RopeXYZ.apply(qkv, xyz.float().contiguous(), inv_freq.float().contiguous(), out_dtype)


class _AttnRope(Function):
    @staticmethod
    def forward(ctx, qkv, xyz, inv_freq, cu_seqlens, max_seqlen, softmax_scale):
        out, lse = ops.attn_rope_fwd(qkv, xyz, inv_freq, cu_seqlens, max_seqlen, softmax_scale)
        ctx.save_for_backward(qkv, out, lse, xyz, inv_freq, cu_seqlens)
        ctx.args = (max_seqlen, softmax_scale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, out, lse, xyz, inv_freq, cu = ctx.saved_tensors
        return ops.attn_rope_bwd(qkv, out, dout.contiguous(), lse, xyz, inv_freq, cu, *ctx.args), None, None, None, None, None


def attn_rope_qkvpacked(qkv: torch.Tensor, xyz: torch.Tensor, inv_freq: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int,
                        softmax_scale: Optional[float] = None, operand_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Point3DRoPE / PointROPE on q and k, then flash_attn_varlen_qkvpacked_func (point_transformer_v3m3_utonia.py:303-323,353-359;
    litept_v1.py:239-265): qkv [n, 3, H, D] UN-rotated -> [n, H, D] in `operand_dtype`.  head_dim 18 with qkv already in the operand
    dtype: ONE operator -- the rotation happens in the attention kernels' prologue and its inverse in their backward epilogue
    (csrc/attention_hd.h ROPE; no rotated copy of q / k in memory).  Anything else (other head dims, an fp16 qkv that the call site
    casts to bf16 AFTER the rotation): the rotation pass ptc_rope3d_xyz followed by the attention kernels -- the same arithmetic."""
    if softmax_scale is None:
        softmax_scale = qkv.shape[-1] ** -0.5
    if (qkv.dtype == operand_dtype and operand_dtype in (torch.bfloat16, torch.float16) and qkv.dim() == 4
            and ops.attn_rope_supported(int(qkv.shape[3]), int(max_seqlen))):
        return _AttnRope.apply(qkv, xyz.float().contiguous(), inv_freq.float().contiguous(), cu_seqlens, int(max_seqlen), float(softmax_scale))
    return attn_varlen_qkvpacked(rope_xyz_qkvpacked(qkv, xyz, inv_freq, operand_dtype), cu_seqlens, max_seqlen, softmax_scale)


# ------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------
class _CrossEntropy(Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        loss_sum, count, lse = ops.cross_entropy_fwd(logits, target, ignore_index)
        ctx.save_for_backward(logits, target, lse, count)
        ctx.ignore_index = ignore_index
        return loss_sum / count          # nan when nothing is counted, as nn.CrossEntropyLoss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logits, target, lse, count = ctx.saved_tensors
        d = ops.cross_entropy_bwd(logits, target, lse, g.float() / count, ctx.ignore_index)
        return d, None, None


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -1, weight=None, label_smoothing: float = 0.0,
                  reduction: str = "mean") -> torch.Tensor:
    """nn.CrossEntropyLoss(ignore_index=ignore_index) (mean over counted points) on seg logits [N, C]
    (pointcept/models/losses/misc.py, pointcept/models/default.py:78-84): one forward and one backward
    kernel, fp32 log-sum-exp straight from the head's (bf16, possibly strided) output.
    With a class `weight` ([C] list or tensor), `label_smoothing` or reduction="sum" the call is the one-term seg_criteria (csrc/criteria.hip;
    up to 1024 classes, element-wise above 32); with all three at their defaults it is exactly the call above."""
    if logits.dim() != 2:
        raise PtcoreError("cross_entropy expects [N, C] logits")
    if weight is None and float(label_smoothing) == 0.0 and reduction == "mean":
        return _CrossEntropy.apply(logits, target, int(ignore_index))
    return seg_criteria(logits, target, [dict(type="CrossEntropyLoss", weight=weight, label_smoothing=label_smoothing, reduction=reduction)],
                        ignore_index)


# ------------------------------------------------------------------------------------------------
# criteria lists: weighted / smoothed cross entropy, Focal and Dice in one pass per direction (csrc/criteria.hip)
# ------------------------------------------------------------------------------------------------
CRITERIA_ROW_TERMS = {      # reference class (losses/misc.py) -> (kernel slot, settings and their defaults)
    "CrossEntropyLoss": ("ce", dict(weight=None, size_average=None, reduce=None, reduction="mean", label_smoothing=0.0)),
    "FocalLoss": ("focal", dict(gamma=2.0, alpha=0.5, reduction="mean")),
    "DiceLoss": ("dice", dict(smooth=1, exponent=2)),
}
CRITERIA_REFUSED = {        # registered by the reference, refused here by name
    "SmoothCELoss": "the reference's SmoothCELoss raises AttributeError (Tensor.total): there is nothing to be faithful to",
    "BinaryFocalLoss": "BinaryFocalLoss takes [N] predictions, not [N, C] seg logits",
}


def criteria_terms(terms, ignore_index=None):
    """The reference's config dicts of row-local terms (type = CrossEntropyLoss | FocalLoss | DiceLoss, loss_weight, ignore_index and
    the class's own settings) -> ([(slot, loss_weight, settings with defaults filled)], ignore_index).  All terms of one call share one
    ignore_index (`ignore_index` overrides the dicts'; default -1).  Refused by name (ValueError): an unknown type or setting,
    SmoothCELoss, BinaryFocalLoss, reduction="none" (and the deprecated size_average / reduce), FocalLoss(reduction="sum") -- which
    raises AttributeError in the reference."""
    out, ignores = [], set()
    for term in terms:
        term = dict(term)
        kind = term.pop("type")
        lw = float(term.pop("loss_weight", 1.0))
        if "ignore_index" in term:
            ignores.add(int(term.pop("ignore_index")))
        if kind in CRITERIA_REFUSED:
            raise ValueError(f"criteria: {kind} is refused: {CRITERIA_REFUSED[kind]}")
        if kind not in CRITERIA_ROW_TERMS:
            raise ValueError(f"criteria: {kind} is not a row-local term of the engine's criteria kernels")
        slot, defaults = CRITERIA_ROW_TERMS[kind]
        unknown = sorted(set(term) - set(defaults))
        if unknown:
            raise ValueError(f"criteria: {kind} has no setting {unknown}")
        s = dict(defaults, **term)
        if slot != "dice" and s["reduction"] not in ("mean", "sum"):
            raise ValueError(f"criteria: {kind}(reduction={s['reduction']!r}) is refused: a per-row loss has no place in a summed criteria list")
        if slot == "ce" and (s["size_average"] is not None or s["reduce"] is not None):
            raise ValueError(f"criteria: {kind} with the deprecated size_average / reduce is refused: say reduction=")
        if slot == "focal":
            if s["reduction"] == "sum":
                raise ValueError("criteria: FocalLoss(reduction='sum') is refused: the reference raises AttributeError (Tensor.total) there")
            if not isinstance(s["gamma"], float) or not (isinstance(s["alpha"], (float, list)) or torch.is_tensor(s["alpha"])):
                raise ValueError("criteria: FocalLoss takes a float gamma and a float or list alpha, as the reference asserts")
        out.append((slot, lw, s))
    if ignore_index is None:
        if len(ignores) > 1:
            raise ValueError(f"criteria: one fused call shares one ignore_index, got {sorted(ignores)}")
        ignore_index = ignores.pop() if ignores else -1
    return out, int(ignore_index)


def _criteria_float(x: torch.Tensor) -> torch.Tensor:
    """the twins compute 16-bit logits in fp32 (the reference's modules run under autocast, where these ops are fp32 too)"""
    return x.float() if x.dtype in (torch.bfloat16, torch.float16) else x


def _criteria_vec(v, like: torch.Tensor, dtype=None):
    return torch.as_tensor(v, dtype=dtype or like.dtype, device=like.device)


def cross_entropy_torch(logits, target, ignore_index: int = -1, weight=None, label_smoothing: float = 0.0, reduction: str = "mean"):
    """misc.py:38-39: nn.CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing).  Labels outside [0, C) are not counted (the
    kernels' rule; ATen asserts on them)."""
    x = _criteria_float(logits)
    t = torch.where((target < 0) | (target >= x.shape[1]), torch.full_like(target, ignore_index), target)
    w = None if weight is None else _criteria_vec(weight, x)
    return F.cross_entropy(x, t, weight=w, ignore_index=int(ignore_index), reduction=reduction, label_smoothing=float(label_smoothing))


def focal_loss_torch(logits, target, gamma: float = 2.0, alpha=0.5, ignore_index: int = -1):
    """FocalLoss(gamma, alpha, reduction="mean", ignore_index).forward (misc.py:123-172) without its loss_weight; labels outside [0, C)
    are not counted (F.one_hot raises on them); with no counted row a zero TENSOR where the reference returns the float 0.0."""
    pred = _criteria_float(logits)
    valid_mask = (target != ignore_index) & (target >= 0) & (target < pred.shape[1])
    target = target[valid_mask]
    pred = pred[valid_mask]
    if target.numel() == 0:
        return pred.sum() * 0
    target = F.one_hot(target, num_classes=pred.size(1))
    if isinstance(alpha, list) or torch.is_tensor(alpha):
        alpha = _criteria_vec(alpha, pred)
    pred_sigmoid = pred.sigmoid()
    target = target.type_as(pred)
    one_minus_pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
    focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * one_minus_pt.pow(gamma)
    return (F.binary_cross_entropy_with_logits(pred, target, reduction="none") * focal_weight).mean()


def dice_loss_torch(logits, target, smooth=1, exponent=2, ignore_index: int = -1):
    """DiceLoss(smooth, exponent, ignore_index).forward (misc.py:188-223) without its loss_weight, quirks included: labels other than
    ignore_index are clamped into [0, C-1]; class i == ignore_index is skipped while the divisor stays C."""
    pred = _criteria_float(logits)
    valid_mask = target != ignore_index
    target = target[valid_mask]
    pred = F.softmax(pred[valid_mask], dim=1)
    num_classes = pred.shape[1]
    target = F.one_hot(torch.clamp(target.long(), 0, num_classes - 1), num_classes=num_classes)
    total_loss = 0
    for i in range(num_classes):
        if i != ignore_index:
            num = torch.sum(torch.mul(pred[:, i], target[:, i])) * 2 + smooth
            den = torch.sum(pred[:, i].pow(exponent) + target[:, i].pow(exponent)) + smooth
            total_loss = total_loss + (1 - num / den)
    return total_loss / num_classes


def _criteria_twin(slot, s, logits, target, ignore_index):
    if slot == "ce":
        return cross_entropy_torch(logits, target, ignore_index, s["weight"], s["label_smoothing"], s["reduction"])
    if slot == "focal":
        return focal_loss_torch(logits, target, s["gamma"], s["alpha"], ignore_index)
    return dice_loss_torch(logits, target, s["smooth"], s["exponent"], ignore_index)


def seg_criteria_torch(logits, target, terms, ignore_index=None):
    """the weighted sum of the terms as the reference computes it (builder.py:22-31 over misc.py's modules)"""
    norm, ignore = criteria_terms(terms, ignore_index)
    loss = 0
    for slot, lw, s in norm:
        loss = loss + _criteria_twin(slot, s, logits, target, ignore) * lw
    return loss


class _SegCriteria(Function):
    @staticmethod
    def forward(ctx, logits, target, spec):
        out, lse, coef = ops.criteria_rows_fwd(logits, target, spec)
        ctx.save_for_backward(logits, target, lse, coef)
        ctx.spec = spec
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logits, target, lse, coef = ctx.saved_tensors
        return ops.criteria_rows_bwd(logits, target, lse, coef, g, ctx.spec), None, None


def _criteria_fill(spec, slot, lw, s, logits):
    if slot == "ce":
        spec.flags |= ops.CRITERIA_CE
        spec.ce_weight = None if s["weight"] is None else _criteria_vec(s["weight"], logits, torch.float32).contiguous()
        spec.ce_eps, spec.ce_sum, spec.ce_lw = float(s["label_smoothing"]), s["reduction"] == "sum", lw
    elif slot == "focal":
        spec.flags |= ops.CRITERIA_FOCAL
        if isinstance(s["alpha"], list) or torch.is_tensor(s["alpha"]):
            spec.focal_alpha_vec = _criteria_vec(s["alpha"], logits, torch.float32).contiguous()
        else:
            spec.focal_alpha = float(s["alpha"])
        spec.focal_gamma, spec.focal_lw = float(s["gamma"]), lw
    else:
        spec.flags |= ops.CRITERIA_DICE
        spec.dice_smooth, spec.dice_exp, spec.dice_lw = float(s["smooth"]), int(s["exponent"]), lw


def seg_criteria(logits: torch.Tensor, target: torch.Tensor, terms, ignore_index=None, use_kernels=None) -> torch.Tensor:
    """The weighted sum of a list of row-local criteria on seg logits [N, C] -- `terms` are the reference's config dicts, see
    criteria_terms -- as ONE autograd Function on csrc/criteria.hip: one forward and one backward kernel read the logits once and write
    dlogits once for the whole list (class-weighted / label-smoothed CrossEntropyLoss with reduction mean | sum, FocalLoss, DiceLoss);
    the means' denominators and Dice's per-class sums stay on the device (no host read), no atomics (bit-reproducible).  A list
    that names one class twice takes one more call for the second instance.
    Kernels: fp32 / bf16 / fp16 logits (any row stride) of up to 32 classes.  The torch twins (*_torch, the reference's expressions)
    serve: FocalLoss and DiceLoss above 32 classes (CrossEntropyLoss stays on the element-wise kernels up to 1024), a DiceLoss exponent
    other than 1 / 2 / 3, float64 logits, CPU tensors, and everything under PTC_CRITERIA=0 (config.CRITERIA_KERNELS).
    Stated difference: FocalLoss with no counted row gives a zero tensor (zero gradient), where the reference returns the float 0.0."""
    if logits.dim() != 2:
        raise PtcoreError("seg_criteria expects [N, C] logits")
    norm, ignore = criteria_terms(terms, ignore_index)
    if use_kernels is None:
        use_kernels = config.CRITERIA_KERNELS and logits.is_cuda
    c = logits.shape[1]
    specs, twins = [], []
    for slot, lw, s in norm:
        on_kernel = (use_kernels and logits.dtype in (torch.float32, torch.bfloat16, torch.float16)
                     and (c <= ops.CRITERIA_ROWS_MAX_C or (slot == "ce" and c <= ops.CRITERIA_CE_MAX_C))
                     and (slot != "dice" or s["exponent"] in (1, 2, 3)))
        if not on_kernel:
            twins.append((slot, lw, s))
            continue
        bit = {"ce": ops.CRITERIA_CE, "focal": ops.CRITERIA_FOCAL, "dice": ops.CRITERIA_DICE}[slot]
        spec = next((sp for sp in specs if not sp.flags & bit), None)
        if spec is None:
            spec = ops.CriteriaSpec(ignore)
            specs.append(spec)
        _criteria_fill(spec, slot, lw, s, logits)
    loss = None
    for spec in specs:
        term = _SegCriteria.apply(logits, target, spec)
        loss = term if loss is None else loss + term
    for slot, lw, s in twins:
        term = _criteria_twin(slot, s, logits, target, ignore) * lw
        loss = term if loss is None else loss + term
    return loss if loss is not None else logits.sum() * 0


def focal_loss(logits, target, gamma: float = 2.0, alpha=0.5, ignore_index: int = -1, use_kernels=None) -> torch.Tensor:
    """FocalLoss(gamma, alpha float | list[C], reduction="mean", ignore_index) (misc.py:96-172) as the one-term seg_criteria; see there
    for the shapes the kernels serve (above 32 classes: the torch twin) and the zero-tensor difference."""
    return seg_criteria(logits, target, [dict(type="FocalLoss", gamma=gamma, alpha=alpha)], ignore_index, use_kernels)


def dice_loss(logits, target, smooth=1, exponent=2, ignore_index: int = -1, use_kernels=None) -> torch.Tensor:
    """DiceLoss(smooth, exponent, ignore_index) (misc.py:175-223) as the one-term seg_criteria; see there for the shapes the kernels
    serve (above 32 classes, or an exponent other than 1 / 2 / 3: the torch twin)."""
    return seg_criteria(logits, target, [dict(type="DiceLoss", smooth=smooth, exponent=exponent)], ignore_index, use_kernels)


class _LovaszSoftmax(Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, present=None):
        # the handle is passed on only when one was given: a three-argument backend (the oracle stand-in) keeps serving the call
        if present is None:
            loss, dlogits = ops.lovasz_softmax(logits, target, ignore_index)
        else:
            loss, dlogits = ops.lovasz_softmax(logits, target, ignore_index, present=present)
        ctx.save_for_backward(dlogits)
        ctx.dtype = logits.dtype
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * g.float()).to(ctx.dtype), None, None, None


def lovasz_present(target: torch.Tensor, num_classes: int, ignore_index: int = -1):
    """The ranked list of the classes present in `target`, made ahead of lovasz_softmax(..., present=handle) (ops.lovasz_present):
    asked for before the backbone runs, the one number the host needs (P) has arrived by the time the loss is called."""
    return ops.lovasz_present(target, int(num_classes), int(ignore_index))


def lovasz_softmax(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -1, present=None) -> torch.Tensor:
    """LovaszLoss(mode="multiclass", ignore_index=ignore_index) on seg logits [N, C], C <= 1024
    (pointcept/models/losses/lovasz.py:209-260; second criterion of scannet/semseg-pt-v3m1-0-base.py:49-52 and of
    scannet200/semseg-pt-v3m1-0-base.py): softmax, per-class errors, ONE segmented sort, exact Jaccard steps and the gradient, all on
    device.  More than 64 classes, or any width with `present` (lovasz_present of the same target): only the classes present are
    sorted; without a handle that path reads their number back once (one host synchronisation)."""
    if logits.dim() != 2:
        raise PtcoreError("lovasz_softmax expects [N, C] logits")
    if present is None:
        return _LovaszSoftmax.apply(logits, target, int(ignore_index))
    return _LovaszSoftmax.apply(logits, target, int(ignore_index), present)


# ------------------------------------------------------------------------------------------------
# BatchNorm1d + activation
# ------------------------------------------------------------------------------------------------
class _BatchNormAct(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, act, res):
        # dense rows for the kernels -- AND for the tensor the backward reads: a Linear / conv output with a channel count that is not a
        # multiple of 16 arrives as a column slice of the padded GEMM output (36 of 48 columns: LitePT; found on hardware in round 3)
        x = x.contiguous()
        if res is not None:
            res = res.contiguous()
        y, mean, rstd = ops.batch_norm_act_fwd(x, weight, bias, running_mean, running_var, training, momentum, eps, act, res=res)
        ctx.save_for_backward(x, weight, bias, mean, rstd, res)
        ctx.training, ctx.act = training, act
        ctx.mark_non_differentiable()
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, bias, mean, rstd, res = ctx.saved_tensors
        out = ops.batch_norm_act_bwd(dy, x, weight, bias, mean, rstd, ctx.training, ctx.act, want_affine=weight is not None, res=res)
        dx, dg, db = out[:3]
        if weight is not None:
            dg, db = dg.to(weight.dtype), db.to(weight.dtype)
        return dx, dg, db, None, None, None, None, None, None, (out[3] if res is not None else None)


def batch_norm_act(x: torch.Tensor, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float,
                   act: str = "none", residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(F.batch_norm(x, ...) [+ residual]) over the rows of [N, C] (act in {"none", "gelu", "relu"}), statistics in
    fp32/fp64, output in x's dtype; backward recomputes the pre-activation (nothing but x and the residual is saved).  With
    `residual` (x's shape and dtype): the tail of a residual block, spconv_unet_v1m1_base.py:79-83, in the BatchNorm's apply pass."""
    return _BatchNormAct.apply(x, weight, bias, running_mean, running_var, bool(training), float(momentum), float(eps), act, residual)


# ------------------------------------------------------------------------------------------------
# one PT-v3m1 Block = ONE autograd Function = one C call per direction (csrc/block_exec.hip)
# ------------------------------------------------------------------------------------------------
_BLK_PARAMS = ("W_CONV", "B_CONV", "W_LIN", "B_LIN", "G_CPE", "BE_CPE", "G_N1", "BE_N1", "W_QKV", "B_QKV", "W_PROJ", "B_PROJ", "G_N2",
               "BE_N2", "W_FC1", "B_FC1", "W_FC2", "B_FC2")
_BLK_WEIGHTS = ("W_CONV", "W_LIN", "W_QKV", "W_PROJ", "W_FC1", "W_FC2")


def _blk_alloc(nbytes, dtype, device):
    """one slab of a Block call: `nbytes` bytes (a multiple of 256) of `dtype`.  Every slab of _BlockFn is allocated here and nowhere else."""
    return torch.empty(nbytes // dtype.itemsize, dtype=dtype, device=device)


_blk_plans = {}


def _blk_plan(E, iv, key):
    """the memory plan of one Block call as csrc/block_exec.hip lays it out (ptc_ptv3_block_layout: host code, no launch), cached
    per key = (n, n_pad, c, heads, dtype of x0, dt): the byte totals of the five slabs and, for the slots this side hands on (dx0,
    dxc, the parameter gradients), where they lie -- name -> (slab, first byte, one past the last)"""
    p = _blk_plans.get(key)
    if p is not None:
        return p
    import ctypes

    totals = (ctypes.c_int64 * E["SLAB_COUNT"])()
    slab, off, size = ((ctypes.c_int64 * E["SLOT_COUNT"])() for _ in range(3))
    if ops.lib().ptc_ptv3_block_layout(iv, totals, slab, off, size) != E["SLOT_COUNT"]:
        raise PtcoreError("ptc_ptv3_block_layout: " + ops.lib().ptc_last_error().decode("utf-8", "replace"))
    cut = {}
    for name in ("G_X0", "G_XC") + tuple("G_" + k for k in _BLK_PARAMS):
        i = E["O_COUNT"] + E[name]
        cut[name] = (slab[i], off[i], off[i] + size[i])
    p = dict(bytes=tuple(totals), cut=cut, ws=None, ws_fwd=None)
    if len(_blk_plans) > 256:
        _blk_plans.clear()
    _blk_plans[key] = p
    return p


def _blk_slab_args(E, slabs):
    """{slab index: tensor} -> the arrays of base pointers and byte sizes the executor's entry points take"""
    import ctypes

    ptrs, sizes = (ctypes.c_void_p * E["SLAB_COUNT"])(), (ctypes.c_int64 * E["SLAB_COUNT"])()
    for i, t in slabs.items():
        ptrs[i], sizes[i] = t.data_ptr(), t.numel() * t.element_size()
    return ptrs, sizes


def _blk_tables(E, x0, meta):
    import ctypes

    n, c = x0.shape
    blk = meta["blk"]
    iv = (ctypes.c_int64 * E["I_COUNT"])()
    iv[E["I_ABI"]], iv[E["I_N"]], iv[E["I_NPAD"]], iv[E["I_NSEQ"]], iv[E["I_C"]] = E["ABI"], n, meta["n_pad"], meta["n_seq"], c
    iv[E["I_HEADS"]], iv[E["I_DTYPE"]], iv[E["I_A_DTYPE"]], iv[E["I_PATCH"]] = (meta["heads"], _lib.PTC_F16 if meta["dt"] == torch.float16 else _lib.PTC_BF16,
                                                                              _lib.dtype_code(x0), meta["patch"])
    iv[E["I_BLK_BM"]], iv[E["I_BLK_HCAP"]] = (0, 0) if blk is None else (blk.bm, blk.hcap)
    fv = (ctypes.c_float * E["F_COUNT"])()
    fv[E["F_SCALE"]], fv[E["F_EPS_CPE"]], fv[E["F_EPS_N1"]], fv[E["F_EPS_N2"]] = meta["scale"], meta["eps_cpe"], meta["eps_n1"], meta["eps_n2"]
    pin = (ctypes.c_void_p * E["P_COUNT"])()
    tabs = meta["tabs"]
    pin[E["P_NBR"]], pin[E["P_CU"]] = meta["nbr"].data_ptr(), meta["cu"].data_ptr()
    pin[E["P_T_QKV_FWD"]], pin[E["P_T_QKV_BWD"]] = tabs[0].data_ptr(), tabs[1].data_ptr()
    pin[E["P_T_PROJ_FWD"]], pin[E["P_T_PROJ_BWD"]] = tabs[2].data_ptr(), tabs[3].data_ptr()
    if blk is not None:
        pin[E["P_BLK_TAB"]], pin[E["P_BLK_HID"]], pin[E["P_BLK_HCNT"]] = blk.tab.data_ptr(), blk.hid.data_ptr(), blk.hcnt.data_ptr()
        if config.WGRAD_BLK:      # (NULL: the executor's convolution weight gradient stays on the global-gather kernel)
            pin[E["P_BLK_NOVF"]] = blk.n_overflow.data_ptr()
    return iv, fv, pin


class _BlockFn(Function):
    """(x3, xb3) = Block(x0, xc): the residual stream after the block (fp32) and its bf16 copy (the operand of the next
    convolution / Linear).  `meta`: sizes, eps, tables (python object, not differentiated); `params`: the block's 18 parameter
    tensors in _BLK_PARAMS order (qkv bias may be None)."""

    @staticmethod
    def forward(ctx, x0, xc, rs1, rs2, meta, *params):
        dt = meta["dt"]            # the autocast dtype of the step: bf16, or f16 (the reference's fp16 recipe)
        n, c = x0.shape
        npad, heads = meta["n_pad"], meta["heads"]
        dev = x0.device
        x0 = x0.contiguous()
        xc = xc.contiguous()
        E = _lib.block_enums()
        iv, fv, pin = _blk_tables(E, x0, meta)
        plan = _blk_plan(E, iv, (n, npad, c, heads, x0.dtype, dt))
        keep = []                                            # tensors the pointer table names (alive until saved / returned)
        for k, p in zip(_BLK_PARAMS, params):
            if p is None:
                continue
            if k in _BLK_WEIGHTS:                            # 16-bit shadows [c_out][taps][c_in] (conv) / [c_out][c_in] (Linear)
                t = _cast_cache.get(p.reshape(p.shape[0], -1, p.shape[-1]) if p.dim() == 5 else p, dt)
            else:
                t = p if p.dtype == torch.float32 else p.float()
            if not t.is_contiguous():
                t = t.contiguous()
            keep.append(t)
            pin[E["P_" + k]] = t.data_ptr()
        pin[E["P_X0"]], pin[E["P_XC"]] = x0.data_ptr(), xc.data_ptr()
        if rs1 is not None:
            pin[E["P_RS1"]] = rs1.data_ptr()
        if rs2 is not None:
            pin[E["P_RS2"]] = rs2.data_ptr()
        # what the backward reads back: two slabs, laid out by the library (16-bit activations; fp32 streams, LayerNorm statistics, lse)
        buf16 = _blk_alloc(plan["bytes"][E["SLAB_SAVED16"]], dt, dev)
        buf32 = _blk_alloc(plan["bytes"][E["SLAB_SAVED32"]], torch.float32, dev)
        pslab, nslab = _blk_slab_args(E, {E["SLAB_SAVED16"]: buf16, E["SLAB_SAVED32"]: buf32})
        x3 = torch.empty((n, c), dtype=torch.float32, device=dev)
        xb3 = torch.empty((n, c), dtype=dt, device=dev)
        if plan["ws_fwd"] is None:
            plan["ws_fwd"] = int(ops.lib().ptc_ptv3_block_fwd_workspace_bytes(n, c))
        nbytes = plan["ws_fwd"]
        # transient (the convolution's fragment-ordered weights at 128 channels and more): NOT saved for the backward
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        ops.lib().ptc_ptv3_block_fwd(iv, fv, pin, pslab, nslab, x3.data_ptr(), xb3.data_ptr(), None if ws is None else ws.data_ptr(), nbytes,
                                     ops.stream_ptr())
        ctx.save_for_backward(x0, xc, rs1, rs2, buf16, buf32, x3, *keep)
        ctx.meta, ctx.plan = meta, plan
        ctx.present = [p is not None for p in params]
        ctx.param_dtypes = [None if p is None else p.dtype for p in params]
        ctx.param_shapes = [None if p is None else p.shape for p in params]
        ctx.set_materialize_grads(False)
        return x3, xb3

    @staticmethod
    @once_differentiable
    def backward(ctx, dz3, dyb3):
        n_par = len(_BLK_PARAMS)
        if dz3 is None and dyb3 is None:
            return (None,) * (5 + n_par)
        sv = ctx.saved_tensors
        x0, xc, rs1, rs2, buf16, buf32, x3 = sv[:7]
        meta, plan = ctx.meta, ctx.plan
        E = _lib.block_enums()
        dt = meta["dt"]
        n, c = x0.shape
        npad, heads = meta["n_pad"], meta["heads"]
        dev = x0.device
        iv, fv, pin = _blk_tables(E, x0, meta)
        it = iter(sv[7:])
        sh = {}
        keep_wt = []
        for k, present in zip(_BLK_PARAMS, ctx.present):
            if present:
                t = next(it)
                pin[E["P_" + k]] = t.data_ptr()
                if k in _BLK_WEIGHTS:
                    sh[k] = t
        # transposed weight layouts of the input-gradient GEMMs (all layers' layouts are refreshed in one launch per step)
        for k, mode, slots in (("CONV", "mirror", 0), ("LIN", "mirror", 0), ("QKV", "repeat", 2), ("PROJ", "mirror", 0), ("FC1", "mirror", 0),
                               ("FC2", "mirror", 0)):
            w = sh["W_" + k]
            wt = _cast_cache.layout(w, mode, slots)
            if wt is None:
                # the shadow is not (or no longer) a cache entry -- a non-leaf / re-parametrised weight, or the cache was invalidated
                # between forward and backward: build this one layout here (the composed path does the same), never fail the step
                w3 = w if w.dim() == 3 else w[:, None, :]
                wt = (w3.flip(1).permute(2, 1, 0) if mode == "mirror" else w3.permute(2, 1, 0).expand(-1, slots, -1)).contiguous()
                keep_wt.append(wt)
            pin[E["P_WT_" + k]] = wt.data_ptr()
        pin[E["P_X0"]], pin[E["P_XC"]] = x0.data_ptr(), xc.data_ptr()
        if rs1 is not None:
            pin[E["P_RS1"]] = rs1.data_ptr()
        if rs2 is not None:
            pin[E["P_RS2"]] = rs2.data_ptr()
        dz3c = None if dz3 is None else (dz3 if dz3.dtype == torch.float32 and dz3.is_contiguous() else dz3.float().contiguous())
        dyb3c = None if dyb3 is None else (dyb3 if dyb3.dtype == dt and dyb3.is_contiguous() else dyb3.to(dt).contiguous())
        if dz3c is not None:
            pin[E["P_DZ3"]] = dz3c.data_ptr()
        if dyb3c is not None:
            pin[E["P_DYB3"]] = dyb3c.data_ptr()
        # parameter gradients in their OWN small slab (~12 C^2 floats): AccumulateGrad keeps the returned views -- and with them their
        # storage -- alive as long as .grad lives; sharing a slab with the 3 N C floats of fp32 scratch pinned ~77 MB per stage-0 Block
        # (ADVICE r3).  The fp32 scratch gradients (and dx0 of an fp32 stream) and the 16-bit ones live in two transient slabs.
        slabs = {E["SLAB_SAVED16"]: buf16, E["SLAB_SAVED32"]: buf32}
        for k, slab_dt in (("SLAB_PGRAD", torch.float32), ("SLAB_SCRATCH32", torch.float32), ("SLAB_SCRATCH16", dt)):
            slabs[E[k]] = _blk_alloc(plan["bytes"][E[k]], slab_dt, dev)
        pslab, nslab = _blk_slab_args(E, slabs)
        if plan["ws"] is None:
            plan["ws"] = int(ops.lib().ptc_ptv3_block_workspace_bytes(n, npad, c, heads))
        nbytes = plan["ws"]
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ops.lib().ptc_ptv3_block_bwd(iv, fv, pin, pslab, nslab, x3.data_ptr(), ws.data_ptr(), nbytes, ops.stream_ptr())

        def cut(name, shape):      # the slot as a view of its slab (G_X0 lies in the slab of x0's dtype)
            slab, lo, hi = plan["cut"][name]
            t = slabs[slab]
            return t[lo // t.element_size():hi // t.element_size()].view(shape)

        dx0, dxc = cut("G_X0", x0.shape), cut("G_XC", x0.shape)
        grads = []
        for k, present, pdt, shp in zip(_BLK_PARAMS, ctx.present, ctx.param_dtypes, ctx.param_shapes):
            if not present:
                grads.append(None)
                continue
            g = cut("G_" + k, shp)
            grads.append(g if pdt == torch.float32 else g.to(pdt))
        return (dx0, dxc, None, None, None, *grads)


def ptv3_block(x0, xc, rs1, rs2, meta, params):
    """One PT-v3m1 Block through csrc/block_exec.hip -> (x3 fp32, xb3 bf16).  See point_transformer_v3.Block._forward_exec."""
    return _BlockFn.apply(x0, xc, rs1, rs2, meta, *params)


# ------------------------------------------------------------------------------------------------
# MLP (fc1 -> GELU -> fc2) with the activation fused into the GEMM epilogues
# ------------------------------------------------------------------------------------------------
class _MLP(Function):
    """out = GELU(x W1^T + b1) W2^T + b2 (ptv3m1:225-248, dropout p = 0).  GELU rides in fc1's epilogue (h and
    GELU(h) leave the kernel together) and GELU' in the epilogue of fc2's input gradient (the gradient reaches
    HBM already multiplied through the activation): the two elementwise kernels of the unfused form, and the
    dA tensor, disappear.  Weight gradients run on the split-K kernels as in `linear`."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        dt = torch.get_autocast_dtype("cuda") if _autocast_on() else x.dtype
        xp = x.to(dt).contiguous()
        w1c, w2c = _cast_cache.get(w1, dt).contiguous(), _cast_cache.get(w2, dt).contiguous()
        ctx.dtypes = (x.dtype, w1.dtype, None if b1 is None else b1.dtype, w2.dtype, None if b2 is None else b2.dtype)
        ctx.one_kernel = w1.shape[0] == 4 * w1.shape[1] and w2.shape[0] == w1.shape[1] and ops.block_mlp_fused(w1.shape[1], dt)
        if ctx.one_kernel:      # round 6 (csrc/mlp.hip): the hidden tensor never reaches memory, the backward recomputes it; same bits as below
            ctx.save_for_backward(xp, w1c, w2c, b1)
            return ops.mlp_fwd(xp, w1c, b1, w2c, b2)
        h, a = ops.linear_gelu_fwd(xp, w1c, b1)
        out = ops.spconv_fwd(a, w2c[:, None, :], None if b2 is None else b2.float(), None)      # shapes: mlp_gelu_supported
        ctx.save_for_backward(xp, h, a, w1c, w2c)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x_dt, w1_dt, b1_dt, w2_dt, b2_dt = ctx.dtypes
        if ctx.one_kernel:
            xp, w1c, w2c, b1 = ctx.saved_tensors
            w2t = _cast_cache.layout(w2c, "mirror")
            dx, dw1, db1, dw2, db2 = ops.mlp_bwd(dout.to(xp.dtype).contiguous(), xp, w1c, b1, w2c.t().contiguous() if w2t is None else w2t[:, 0, :],
                                                 want_b1=b1_dt is not None, want_b2=b2_dt is not None)
            return (dx.to(x_dt) if ctx.needs_input_grad[0] else None, dw1.to(w1_dt), None if db1 is None else db1.to(b1_dt), dw2.to(w2_dt),
                    None if db2 is None else db2.to(b2_dt))
        xp, h, a, w1c, w2c = ctx.saved_tensors
        g = dout.to(xp.dtype).contiguous()
        n = g.shape[0]
        # fc2: weight / bias gradients, then the input gradient THROUGH the activation
        res = ops.spconv_wgrad(a, g, None, want_bias=b2_dt is not None)
        dw2, db2 = res if b2_dt is not None else (res, None)
        dw2 = dw2[:, 0, :]
        dw2 = dw2.to(w2_dt)
        db2 = None if db2 is None else db2.to(b2_dt)
        w2t = _cast_cache.layout(w2c, "mirror")
        dh = ops.linear_gelu_bwd_input(g, w2c.t().contiguous() if w2t is None else w2t[:, 0, :], h)
        # fc1: the same split
        res = ops.spconv_wgrad(xp, dh, None, want_bias=b1_dt is not None)
        dw1, db1 = res if b1_dt is not None else (res, None)
        dw1 = dw1[:, 0, :]
        dw1 = dw1.to(w1_dt)
        db1 = None if db1 is None else db1.to(b1_dt)
        dx = None
        if ctx.needs_input_grad[0]:
            w1t = _cast_cache.layout(w1c, "mirror")
            dx = ops.spconv_fwd(dh, w1c.t().contiguous()[:, None, :] if w1t is None else w1t, None, None).to(x_dt)
        return dx, dw1, db1, dw2, db2


def mlp_gelu_supported(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> bool:
    if not (x.is_cuda and x.dim() == 2 and x.shape[0] > 0):
        return False
    dt = torch.get_autocast_dtype("cuda") if _autocast_on() else x.dtype
    hidden, c = w1.shape
    # (fc2 and fc1's input gradient contract over `hidden`: beyond linear2's 256 channels they run on the identity-table kernel, which
    #  wants 32-channel multiples on both sides -- other widths take the unfused Linear -> GELU -> Linear, whose operands are padded)
    return (dt in (torch.bfloat16, torch.float16) and c % 16 == 0 and hidden % 16 == 0 and w2.shape[0] % 16 == 0
            and ops.linear_supported_ex(c, hidden, dt) and ops.linear_supported_ex(w2.shape[0], hidden, dt)
            and _own_gemm(0, hidden, dt, w2.shape[0]) and _own_gemm(0, hidden, dt, c))


def mlp_gelu(x, w1, b1, w2, b2):
    return _MLP.apply(x, w1, b1, w2, b2)


# ------------------------------------------------------------------------------------------------
# OA-CNNs adaptive aggregation (csrc/cluster_agg.hip)
# ------------------------------------------------------------------------------------------------
class _ClusterCenter(Function):
    @staticmethod
    def forward(ctx, gc, *xs):
        ctx.gc = gc
        return tuple(ops.cluster_center(list(xs), gc))

    @staticmethod
    @once_differentiable
    def backward(ctx, *gys):
        # y = x - mean_c(x)[c] is a symmetric projection: its backward is the same operator on dy
        gys = [g.contiguous() if g is not None else None for g in gys]
        if any(g is None for g in gys):
            ref = next(g for g in gys if g is not None)
            gys = [torch.zeros_like(ref) if g is None else g for g in gys]
        return (None, *ops.cluster_center(gys, ctx.gc))


def cluster_center(xs, gc: "ops.GridClusters") -> list:
    """[x_l - scatter(x_l, cluster_l, reduce="mean")[cluster_l] for every level] (oacnns_v1m1_base.py:92) in one launch per pass."""
    dt = xs[0].dtype
    return list(_ClusterCenter.apply(gc, *[x.to(dt).contiguous() for x in xs]))


class _ClusterAgg(Function):
    @staticmethod
    def forward(ctx, gc, a, *uv):
        L = gc.levels
        us, vs = list(uv[:L]), list(uv[L:])
        out, state = ops.cluster_agg_fwd(us, vs, a, gc)
        ctx.gc = gc
        ctx.save_for_backward(a, state, *us, *vs)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        a, state, *uv = ctx.saved_tensors
        L = ctx.gc.levels
        du, dv, da = ops.cluster_agg_bwd(uv[:L], uv[L:], a, dout, state, ctx.gc)
        return (None, da, *du, *dv)


def cluster_agg(us, vs, a: torch.Tensor, gc: "ops.GridClusters") -> torch.Tensor:
    """sum_l softmax(a)_l * scatter(v_l * pw_l, cluster_l)[cluster_l],  pw_l = e_l / (scatter(e_l, cluster_l)[cluster_l] + 1e-6),
    e_l = exp(u_l - u_l.max())  (oacnns_v1m1_base.py:93-102) on csrc/cluster_agg.hip.  Operands are taken in the dtype of u_0 (the
    16-bit type under autocast); arithmetic is fp32."""
    dt = us[0].dtype
    c = lambda t: t.to(dt).contiguous()   # noqa: E731
    return _ClusterAgg.apply(gc, c(a), *[c(u) for u in us], *[c(v) for v in vs])


def cluster_center_torch(xs, gc: "ops.GridClusters") -> list:
    """PTC_OACNN_AGG=0: the reference's expression of :92 (ATen index_add scatter)."""
    out = []
    for x, cl, n_c in zip(xs, gc.cluster, gc.n_cluster):
        s = x.new_zeros((n_c, x.shape[1])).index_add(0, cl, x)
        cnt = torch.bincount(cl, minlength=n_c).clamp(min=1).to(x.dtype)
        out.append(x - (s / cnt[:, None])[cl])
    return out


def cluster_agg_torch(us, vs, a: torch.Tensor, gc: "ops.GridClusters") -> torch.Tensor:
    """PTC_OACNN_AGG=0: the reference's expression of :93-102 (ATen exp / index_add / softmax / einsum)."""
    feats = []
    for u, v, cl, n_c in zip(us, vs, gc.cluster, gc.n_cluster):
        pw = torch.exp(u - u.max())
        pw = pw / (pw.new_zeros((n_c, pw.shape[1])).index_add(0, cl, pw)[cl] + 1e-6)
        pf = v * pw
        feats.append(pf.new_zeros((n_c, pf.shape[1])).index_add(0, cl, pf)[cl])
    adp = torch.softmax(a, dim=1)
    return torch.einsum("l n, l n c -> l c", adp, torch.stack(feats, dim=1))


# ------------------------------------------------------------------------------------------------
# PointGroup (point_group_v1m1_base.py:72-91): masked L1 + negative-cosine offset losses, one fused pass each way
# ------------------------------------------------------------------------------------------------
class _PGBiasLoss(Function):
    @staticmethod
    def forward(ctx, bias_pred, coord, centroid, instance, ignore_index):
        out = ops.pg_bias_loss_fwd(bias_pred, coord, centroid, instance, ignore_index)
        ctx.save_for_backward(bias_pred, coord, centroid, instance, out)
        ctx.ignore_index = ignore_index
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_l1, g_cos):
        bias_pred, coord, centroid, instance, out = ctx.saved_tensors
        z = torch.zeros((), dtype=torch.float32, device=bias_pred.device)
        dout = torch.stack([z if g_l1 is None else g_l1.float().reshape(()), z if g_cos is None else g_cos.float().reshape(())])
        d = ops.pg_bias_loss_bwd(bias_pred, coord, centroid, instance, ctx.ignore_index, dout, out)
        return d, None, None, None, None


def pg_bias_loss(bias_pred: torch.Tensor, coord: torch.Tensor, centroid: torch.Tensor, instance: torch.Tensor, ignore_index: int = -1):
    """(bias_l1_loss, bias_cosine_loss) of point_group_v1m1_base.py:72-91 with bias_gt = centroid - coord; fp32 scalars"""
    return _PGBiasLoss.apply(bias_pred, coord, centroid, instance, int(ignore_index))


def pg_bias_loss_torch(bias_pred, coord, centroid, instance, ignore_index: int = -1):
    """the reference's expression (point_group_v1m1_base.py:72-91), for A/B"""
    mask = (instance != ignore_index).float()
    bias_gt = centroid - coord
    bias_dist = torch.sum(torch.abs(bias_pred - bias_gt), dim=-1)
    l1 = torch.sum(bias_dist * mask) / (torch.sum(mask) + 1e-8)
    pn = bias_pred / (torch.norm(bias_pred, p=2, dim=1, keepdim=True) + 1e-8)
    gn = bias_gt / (torch.norm(bias_gt, p=2, dim=1, keepdim=True) + 1e-8)
    cos = -(pn * gn).sum(-1)
    return l1, torch.sum(cos * mask) / (torch.sum(mask) + 1e-8)


def pg_ball_query_torch(xyz: torch.Tensor, batch_idxs: torch.Tensor, batch_offsets, radius: float, chunk: int = 256):
    """ballquery_batch_p as chunked brute-force torch (the A/B baseline and cross-check of csrc/pg_cluster.hip): the reference's
    unfused d2 < radius^2, ascending neighbours, the first 1000 kept -> (idx int32, start_len int32 [n, 2])"""
    x = xyz.float().contiguous()
    n = x.shape[0]
    off = [int(v) for v in torch.as_tensor(batch_offsets).tolist()]
    bidx = batch_idxs.long()
    r2 = float(torch.tensor(radius, dtype=torch.float32) * torch.tensor(radius, dtype=torch.float32))   # fp32 radius * radius
    lens = torch.zeros(n, dtype=torch.int64, device=x.device)
    pieces = []
    for q0 in range(0, n, chunk):
        q1 = min(n, q0 + chunk)
        qb = bidx[q0:q1]
        bs = sorted(set(qb.tolist()))
        for b in bs:
            rows = torch.nonzero(qb == b)[:, 0] + q0
            s, e = off[b], off[b + 1]
            o, seg = x[rows], x[s:e]
            dx = o[:, None, 0] - seg[None, :, 0]
            dy = o[:, None, 1] - seg[None, :, 1]
            dz = o[:, None, 2] - seg[None, :, 2]
            d2 = dx * dx + dy * dy
            d2 = d2 + dz * dz
            hit = d2 < r2
            hit &= torch.cumsum(hit.to(torch.int32), dim=1) <= ops.PG_MAX_NEIGHBOURS
            lens[rows] = hit.sum(1)
            rr, kk = torch.nonzero(hit, as_tuple=True)
            pieces.append((rows[rr], kk + s))
    if pieces:
        rows = torch.cat([p[0] for p in pieces])
        ks = torch.cat([p[1] for p in pieces])
        o = torch.argsort(rows * (n + 1) + ks)
        idx = ks[o].to(torch.int32)
    else:
        idx = torch.zeros(0, dtype=torch.int32, device=x.device)
    starts = torch.cumsum(lens, 0) - lens
    return idx, torch.stack([starts, lens], 1).to(torch.int32)


def pg_bfs_cluster_host(label, idx, start_len, threshold: int):
    """bfs_cluster.cpp:53-123 on the host (the A/B baseline): CPU int32 tensors, members in BFS order"""
    from collections import deque

    lab = label.cpu().numpy()
    ix = idx.cpu().numpy()
    sl = start_len.cpu().numpy()
    n = sl.shape[0]
    visited = bytearray(n)
    rows, offs = [], [0]
    for i in range(n):
        if visited[i]:
            continue
        cc = [i]
        visited[i] = 1
        q = deque(cc)
        while q:
            cur = q.popleft()
            s, ln, lc = sl[cur, 0], sl[cur, 1], lab[cur]
            for j in ix[s:s + ln].tolist():
                if visited[j] or lab[j] != lc:
                    continue
                visited[j] = 1
                cc.append(j)
                q.append(j)
        if len(cc) >= threshold:
            rows.append(cc)
            offs.append(offs[-1] + len(cc))
    import numpy as np

    cidx = np.zeros((offs[-1], 2), dtype=np.int32)
    for k, cc in enumerate(rows):
        cidx[offs[k]:offs[k + 1], 0] = k
        cidx[offs[k]:offs[k + 1], 1] = cc
    return torch.from_numpy(cidx), torch.tensor(offs, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------
# Masked Scene Contrast (masked_scene_contrast_v1m1_base.py:144-203): matching and the fused InfoNCE loss
# ------------------------------------------------------------------------------------------------
class _MSCNce(Function):
    @staticmethod
    def forward(ctx, feat1, feat2, match_index, nce_t):
        out, state = ops.msc_nce_fwd(feat1, feat2, match_index, nce_t)
        ctx.save_for_backward(*state)
        ctx.shape = (feat1.shape[0], feat2.shape[0], float(nce_t))
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_loss, g_pos, g_neg):
        n1, n2, nce_t = ctx.shape
        if g_loss is None:
            return None, None, None, None
        d1, d2 = ops.msc_nce_bwd(tuple(ctx.saved_tensors), n1, n2, nce_t, g_loss)
        return d1, d2, None, None


def msc_nce(feat1: torch.Tensor, feat2: torch.Tensor, match_index: torch.Tensor, nce_t: float):
    """(nce loss, pos_sim, neg_sim) of compute_contrastive_loss (:179-193) on the fused kernels: fp32 scalars, the loss
    differentiable in feat1 / feat2, the two similarities detached as there.  16-bit features are cast up (the config's recipe is
    fp32, enable_amp = False)."""
    with torch.autocast(device_type=feat1.device.type, enabled=False):
        loss, pos, neg = _MSCNce.apply(feat1.float(), feat2.float(), match_index, float(nce_t))
    return loss, pos.detach(), neg.detach()


def msc_nce_torch(feat1, feat2, match_index, nce_t: float):
    """the reference's expression (:179-193): gather, normalise, the dense P x P similarity matrix, CrossEntropy (A/B and CPU path)"""
    a = feat1[match_index[:, 0]]
    b = feat2[match_index[:, 1]]
    a = a / (torch.norm(a, p=2, dim=1, keepdim=True) + 1e-7)
    b = b / (torch.norm(b, p=2, dim=1, keepdim=True) + 1e-7)
    sim = torch.mm(a, b.transpose(1, 0))
    with torch.no_grad():
        pos_sim = torch.diagonal(sim).mean()
        neg_sim = sim.mean(dim=-1).mean() - pos_sim / match_index.shape[0]
    labels = torch.arange(sim.shape[0], device=a.device).long()
    loss = torch.nn.functional.cross_entropy(torch.div(sim, nce_t), labels, reduction="mean")
    return loss, pos_sim, neg_sim


class _MSCCscNce(Function):
    @staticmethod
    def forward(ctx, feat1, coord1, offset1, feat2, coord2, match_index, nce_t, r1, r2, partitions):
        out, _, state = ops.msc_csc_nce_fwd(feat1, coord1, offset1, feat2, coord2, match_index, nce_t, r1, r2, partitions)
        ctx.save_for_backward(*state)
        ctx.shape = (feat1.shape[0], feat2.shape[0], float(nce_t), float(r1), float(r2))
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_loss, g_pos, g_neg):
        n1, n2, nce_t, r1, r2 = ctx.shape
        if g_loss is None:
            return (None,) * 10
        d1, d2 = ops.msc_csc_nce_bwd(tuple(ctx.saved_tensors), n1, n2, nce_t, r1, r2, g_loss)
        return d1, None, None, d2, None, None, None, None, None, None


def msc_csc_nce(feat1, coord1, offset1, feat2, coord2, match_index, nce_t: float, r1: float, r2: float, partitions: int = 4):
    """(nce loss, pos_sim, neg_sim) of MSC-v1m2's compute_contrastive_loss (masked_scene_contrast_v1m2_csc.py:212-254) on the fused
    kernels: one InfoNCE per scene and partition class of rel = x1[j] - x2[i], summed over the classes present in the scene and
    divided by (scenes * partitions).  match_index in any row order; no P_b x P_b tensor and no host read.  fp32 scalars, the loss
    differentiable in feat1 / feat2, the two similarities detached; 16-bit features are cast up (enable_amp = False in the recipe)."""
    with torch.autocast(device_type=feat1.device.type, enabled=False):
        loss, pos, neg = _MSCCscNce.apply(feat1.float(), coord1.float(), offset1, feat2.float(), coord2.float(), match_index, float(nce_t),
                                          float(r1), float(r2), int(partitions))
    return loss, pos.detach(), neg.detach()


def msc_csc_partitions(coord1, coord2, r1: float, r2: float):
    """compute_partitions (:182-200) on fp32 coordinates: [len(coord2), len(coord1)] classes 0..3 and -1e7 for the rest; element
    (i, j) is the class of coord1[j] - coord2[i]"""
    coord1, coord2 = coord1.float(), coord2.float()
    rel = coord1.unsqueeze(0) - coord2.unsqueeze(1)
    up, down = rel[:, :, 2] > 0.0, rel[:, :, 2] < 0.0
    dist = torch.sqrt(torch.sum(rel.pow(2), 2).add(1e-7))
    part = torch.full(dist.shape, -1e7, device=coord1.device)
    mid, far = (dist > r1) & (dist <= r2), dist > r2
    part[mid & up] = 0
    part[mid & down] = 1
    part[far & up] = 2
    part[far & down] = 3
    return part


def msc_csc_nce_torch(feat1, coord1, offset1, feat2, coord2, match_index, nce_t: float, r1: float, r2: float, partitions: int = 4):
    """the reference's expression (:212-254): a host loop over the scenes that hold pairs, the dense P_b x P_b similarity and
    partition matrices, one masked CrossEntropy per class present (A/B and CPU path).  The partitions always come from
    coord.float(), so a float64 run of the features sees the classes of the fp32 run."""
    from .structure import offset2batch

    a = feat1[match_index[:, 0]]
    b = feat2[match_index[:, 1]]
    a = a / (torch.norm(a, p=2, dim=1, keepdim=True) + 1e-7)
    b = b / (torch.norm(b, p=2, dim=1, keepdim=True) + 1e-7)
    x1, x2 = coord1[match_index[:, 0]], coord2[match_index[:, 1]]
    loss = torch.zeros((), dtype=a.dtype, device=a.device)
    pos_sim, neg_sim = torch.zeros_like(loss), torch.zeros_like(loss)
    batch = offset2batch(offset1)[match_index[:, 0]]
    for batch_id in batch.unique():
        sel = batch == batch_id
        sim = torch.mm(a[sel], b[sel].transpose(1, 0))
        with torch.no_grad():
            pos_sim += torch.diagonal(sim).mean()
            neg_sim += sim.mean(dim=-1).mean() - pos_sim / sel.sum()
        labels = torch.arange(sim.shape[0], device=a.device).long()
        part = msc_csc_partitions(x1[sel], x2[sel], r1, r2)
        for part_id in part.unique():
            keep = part == part_id
            keep.fill_diagonal_(True)
            loss = loss + torch.nn.functional.cross_entropy(torch.div(sim, nce_t) - 1e9 * (~keep).to(sim.dtype), labels, reduction="mean")
    n_scenes = len(offset1)
    return loss / (n_scenes * partitions), pos_sim / n_scenes, neg_sim / n_scenes


def msc_candidates_torch(k: int, max_radius: float, xyz, offset, new_xyz, new_offset):
    """(count, cand) of ops.msc_match written as the reference writes it: knn_query, then `distance < max_radius` (:147-162)"""
    idx, dist = ops.knn_query(k, xyz.float(), offset.int(), new_xyz.float(), new_offset.int())
    keep = dist < max_radius
    return keep.sum(1).to(torch.int32), torch.where(keep, idx, torch.full_like(idx, -1))


def msc_select_torch(count: torch.Tensor, cand: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """:154-169 on (count, cand): the compacted (query, candidate) list, unique's counts, cumsum(count) - r % count - 1"""
    k = cand.shape[1]
    index = torch.cat([torch.arange(cand.shape[0], device=cand.device, dtype=torch.long).view(-1, 1, 1).expand(-1, k, 1),
                       cand.long().view(-1, k, 1)], dim=-1)[cand >= 0]
    _, cnt = index[:, 0].unique(return_counts=True)
    select = torch.cumsum(cnt, dim=0) - r.to(cnt.device) % cnt - 1
    return index[select]


# ------------------------------------------------------------------------------------------------
# Context-aware classifier (context_aware_classifier_v1m1_base.py): prototype pooling, cosine classifier, distillation loss.
# Each kernel Function has a *_torch twin: the reference's own expression, loops included, device-neutral -- the A/B baseline
# (PTC_CAC=0), the CPU path, and what the wrapper takes for shapes the kernels refuse.
# ------------------------------------------------------------------------------------------------
def _cac_bounds(offset, n):
    if offset is None:
        return [(0, n)]
    ends = [int(e) for e in offset.tolist()]
    return list(zip([0] + ends[:-1], ends))


class _CACPoolSoft(Function):
    @staticmethod
    def forward(ctx, x, logits, offset, conf_thresh, eps):
        x, logits = x.contiguous(), logits.contiguous()
        proto, wsum, _, passed = ops.cac_pool_fwd(x, logits=logits, offset=offset, conf_thresh=conf_thresh, eps=eps)
        ctx.save_for_backward(x, logits, proto, wsum)
        ctx.args = (offset, float(conf_thresh), float(eps))
        ctx.mark_non_differentiable(wsum, passed)
        return proto, wsum, passed

    @staticmethod
    @once_differentiable
    def backward(ctx, dproto, _dw, _dp):
        x, logits, proto, wsum = ctx.saved_tensors
        offset, thresh, eps = ctx.args
        dx, dl = ops.cac_pool_bwd(x, logits, None, offset, thresh, eps, proto, wsum, dproto, ctx.needs_input_grad[1])
        return (dx if ctx.needs_input_grad[0] else None), dl, None, None, None


def cac_pool_soft(x, logits, offset=None, conf_thresh: float = 0.0, eps: float = 1e-7):
    """(proto [S, K, C], wsum [S, K], passed [S]) of post_refine_proto_batch (:111-117, :134-142) for all scenes at once:
    proto[s] = (p / (p.sum(-1) + eps)) @ x over the rows of scene s, p = softmax(logits) times the confidence gate.  Differentiable
    in x and logits.  fp32 kernels: 16-bit inputs are cast up."""
    with torch.autocast(device_type=x.device.type, enabled=False):
        return _CACPoolSoft.apply(x.float(), logits.float(), offset, float(conf_thresh), float(eps))


def cac_pool_soft_torch(x, logits, offset=None, conf_thresh: float = 0.0, eps: float = 1e-7):
    protos, sums, passed = [], [], []
    for start, end in _cac_bounds(offset, x.shape[0]):
        pred = F.softmax(logits[start:end], 1).permute(1, 0)
        if conf_thresh > 0:
            max_pred = (pred.max(0)[0] >= conf_thresh).to(pred.dtype).unsqueeze(0)
            passed.append(max_pred.sum())
            pred = pred * max_pred
        else:
            passed.append(torch.as_tensor(float(end - start), device=x.device))
        sums.append(pred.sum(-1))
        protos.append((pred / (pred.sum(-1).unsqueeze(-1) + eps)) @ x[start:end])
    return torch.stack(protos), torch.stack(sums).detach(), torch.stack(passed).long()


class _CACPoolHard(Function):
    @staticmethod
    def forward(ctx, x, target, num_classes, eps):
        proto, wsum, count, _ = ops.cac_pool_fwd(x, target=target, num_classes=num_classes, eps=eps)
        ctx.save_for_backward(x, target.to(torch.int64).contiguous(), proto, wsum)
        ctx.eps = float(eps)
        ctx.mark_non_differentiable(count)
        return proto[0], count

    @staticmethod
    @once_differentiable
    def backward(ctx, dproto, _dc):
        x, target, proto, wsum = ctx.saved_tensors
        dx, _ = ops.cac_pool_bwd(x, None, target, None, 0.0, ctx.eps, proto, wsum, dproto.unsqueeze(0), False)
        return dx, None, None, None


def cac_pool_hard(x, target, base, eps: float = 1e-4):
    """(new_proto [K, C], count [K]) of get_adaptive_perspective's class loop (:78-90): the rows of `base` whose class occurs in
    `target` replaced by sum_{target == k} x / (count_k + eps); rows with target -1 take no part; absent classes keep their row."""
    with torch.autocast(device_type=x.device.type, enabled=False):
        proto, count = _CACPoolHard.apply(x.float(), target, base.shape[0], float(eps))
        return torch.where((count > 0).unsqueeze(-1), proto, base.float()), count


def cac_pool_hard_torch(x, target, base, eps: float = 1e-4):
    new_proto = base
    unique_y = [y for y in target.unique() if int(y) != -1]
    t = target.unsqueeze(-1)
    for tmp_y in unique_y:
        tmp_mask = (t == tmp_y).to(x.dtype)
        tmp_proto = (x * tmp_mask).sum(0) / (tmp_mask.sum(0) + eps)
        onehot_vec = torch.zeros(new_proto.shape[0], 1, dtype=x.dtype, device=x.device)
        onehot_vec[tmp_y.long()] = 1
        new_proto = new_proto * (1 - onehot_vec) + tmp_proto.unsqueeze(0) * onehot_vec
    count = torch.bincount(target[target >= 0], minlength=base.shape[0])
    return new_proto, count


class _CACCos(Function):
    @staticmethod
    def forward(ctx, x, proto, offset, cos_temp):
        ctx.save_for_backward(x, proto)
        ctx.args = (offset, float(cos_temp))
        return ops.cac_cos_fwd(x, proto, offset, cos_temp)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, proto = ctx.saved_tensors
        offset, cos_temp = ctx.args
        dx, dp = ops.cac_cos_bwd(x, proto, offset, cos_temp, dout)
        return dx, dp, None, None


def cac_cos_logits(x, proto, offset=None, cos_temp: float = 1.0):
    """get_pred (:66-71) times cos_temp for all scenes at once: out[i] = cos_temp * normalize(x_i) @ normalize(proto[s(i)]).T with
    proto [S, K, C] (or [K, C]: one set for every row).  Differentiable in x and proto.  fp32 kernels: 16-bit inputs are cast up."""
    with torch.autocast(device_type=x.device.type, enabled=False):
        p = proto.float()
        return _CACCos.apply(x.float(), p.unsqueeze(0) if p.dim() == 2 else p, offset if proto.dim() == 3 else None, float(cos_temp))


def cac_cos_logits_torch(x, proto, offset=None, cos_temp: float = 1.0):
    if proto.dim() == 2:
        return F.normalize(x, 2, 1) @ F.normalize(proto, 2, 1).permute(1, 0) * cos_temp
    out = [F.normalize(x[start:end], 2, 1) @ F.normalize(proto[i], 2, 1).permute(1, 0)
           for i, (start, end) in enumerate(_cac_bounds(offset, x.shape[0]))]
    return torch.cat(out, 0) * cos_temp


class _CACDistill(Function):
    @staticmethod
    def forward(ctx, pred, soft, target, smoothness, eps):
        loss, stats, state = ops.cac_distill_fwd(pred, soft, target, smoothness, eps)
        ctx.save_for_backward(stats, *state)
        ctx.args = (float(smoothness), float(eps))
        return loss[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        stats, pred, soft, tg = ctx.saved_tensors
        return ops.cac_distill_bwd((pred, soft, tg), ctx.args[0], ctx.args[1], stats, dloss), None, None, None, None


def cac_distill(pred, soft, target, smoothness: float = 0.5, eps: float = 0):
    """get_distill_loss (:152-199): class-wise entropy-weighted distillation of softmax(soft) (detached) into pred; a scalar,
    differentiable in pred.  fp32 kernels: 16-bit inputs are cast up."""
    with torch.autocast(device_type=pred.device.type, enabled=False):
        return _CACDistill.apply(pred.float(), soft.detach().float(), target, float(smoothness), float(eps))


def cac_distill_torch(pred, soft, target, smoothness: float = 0.5, eps: float = 0):
    n, c = soft.shape[:]
    soft = soft.detach()
    target = target.unsqueeze(-1)
    onehot = target.view(-1, 1)
    ignore_mask = (onehot == -1).to(soft.dtype)
    sm_soft = F.softmax(soft / 1, 1)
    onehot = onehot * (1 - ignore_mask)
    onehot = torch.zeros(n, c, dtype=soft.dtype, device=soft.device).scatter_(1, onehot.long(), 1)
    smoothed_label = smoothness * sm_soft + (1 - smoothness) * onehot
    if eps > 0:
        smoothed_label = smoothed_label * (1 - eps) + (1 - smoothed_label) * eps / (smoothed_label.shape[1] - 1)
    loss = torch.mul(-1 * F.log_softmax(pred, dim=1), smoothed_label)
    loss = loss.sum(1)
    sm_soft = F.softmax(soft / 1, 1)
    entropy_mask = -1 * (sm_soft * torch.log(sm_soft + 1e-4)).sum(1)
    target = target.squeeze(-1)
    unique_classes = [y for y in target.unique() if int(y) != -1]
    valid_mask = (target != -1).to(soft.dtype)
    entropy_mask = entropy_mask * valid_mask
    loss_list = []
    weight_list = []
    for tmp_y in unique_classes:
        tmp_mask = (target == tmp_y).to(soft.dtype).squeeze()
        tmp_entropy_mask = entropy_mask * tmp_mask
        class_weight = 1
        tmp_loss = (loss * tmp_entropy_mask).sum() / (tmp_entropy_mask.sum() + 1e-4)
        loss_list.append(class_weight * tmp_loss)
        weight_list.append(class_weight)
    if len(weight_list) > 0:
        return sum(loss_list) / (sum(weight_list) + 1e-4)
    return torch.zeros(1, dtype=pred.dtype, device=pred.device).mean()


# ------------------------------------------------------------------------------------------------
# Point Prompt Training's language-guided head (point_prompt_training_v1m1_language_guided.py:98-107, _v1m3_neo.py:117-129)
# ------------------------------------------------------------------------------------------------
def _ppt_scale(logit_scale) -> float:
    """exp(logit_scale) as a host float (a tensor costs one device read; point_prompt_training.py caches it per parameter version)"""
    if isinstance(logit_scale, torch.Tensor):
        return float(logit_scale.detach().float().exp())
    return math.exp(float(logit_scale))


class _PPTHead(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, e, logit_scale, scale, eps):
        dt = _autocast_dtype(x)
        with torch.autocast(device_type=x.device.type, enabled=False):
            xc = x.to(dt).contiguous()
            wc = _cast_cache.get(weight, dt).contiguous()
            b32 = (bias.float() if bias is not None else torch.zeros(weight.shape[0], dtype=torch.float32, device=x.device)).contiguous()
            e32 = e.float().contiguous()
            logits, inv = ops.ppt_head_fwd(xc, wc, b32, e32, scale, eps)
        ctx.save_for_backward(xc, weight, bias, e32, logits, inv, logit_scale if isinstance(logit_scale, torch.Tensor) else None)
        ctx.args = (float(scale), float(eps), x.dtype)
        ctx.mark_non_differentiable(inv)
        return logits, inv

    @staticmethod
    @once_differentiable
    def backward(ctx, dlogits, _dinv):
        xc, weight, bias, e32, logits, inv, logit_scale = ctx.saved_tensors
        scale, eps, in_dtype = ctx.args
        need = ctx.needs_input_grad
        dx = dw = db = ds = None
        with torch.autocast(device_type=xc.device.type, enabled=False):
            dl = dlogits.float().contiguous()
            if need[4] and logit_scale is not None:          # d / d logit_scale of exp(logit_scale) * sim
                ds = (dl * logits).sum().to(logit_scale.dtype).reshape(logit_scale.shape)
            if need[0] or need[1] or need[2]:
                # the small fp32 products around the kernel: [<= 1024, <= 128] matrices
                w32 = weight.detach().float()
                b32 = bias.detach().float() if bias is not None else torch.zeros(w32.shape[0], dtype=torch.float32, device=w32.device)
                w64 = w32.double()          # M x + u cancels where h is small against |W| |x|: formed (and used by the kernel) in double
                G, M, u = e32 @ w32, w64.t() @ w64, w64.t() @ b32.double()
                dxc, A, Bm, v, asum, rsum = ops.ppt_head_bwd(xc, dl, logits, inv, G, M, u, w32.shape[0], scale, eps)
                if need[0]:
                    dx = dxc.to(in_dtype)
                if need[1]:
                    dw = (e32.t() @ A - w32 @ Bm - torch.outer(b32, v)).to(weight.dtype)
                if need[2] and bias is not None:
                    db = (e32.t() @ asum - w32 @ v - b32 * rsum).to(bias.dtype)
        return dx, dw, db, None, ds, None, None          # the class rows arrive detached (a trainable embedding takes ppt_head_torch)


def ppt_head_kernels(x: torch.Tensor, weight: torch.Tensor, class_embedding: torch.Tensor, use_kernels=None) -> bool:
    """whether functional.ppt_head runs csrc/ppt.hip for these operands (else: functional.ppt_head_torch)"""
    want = bool(config.PPT_KERNELS and x.is_cuda) if use_kernels is None else bool(use_kernels)
    if not want or x.dim() != 2 or x.shape[0] == 0 or class_embedding.requires_grad:
        return False
    dt = _autocast_dtype(x)
    return dt in (torch.float32, torch.bfloat16, torch.float16) and ops.ppt_head_supported(x.shape[1], weight.shape[0], class_embedding.shape[0], dt)


def ppt_head(x, weight, bias, class_embedding, logit_scale, eps: float = 0.0, return_inv_norm: bool = False, use_kernels=None):
    """seg_logits [N, K] = exp(logit_scale) * normalize(x @ weight.T + bias) @ class_embedding.T of PPT-v1m1 (:98-107, eps = 0: a
    plain division by the norm) and PPT-v1m3 (:117-129, F.normalize's eps), with class_embedding [K, D] the rows already selected.
    One kernel per direction (csrc/ppt.hip): the [N, D] projection lives in registers, nothing D-wide is stored or revisited by the
    backward.  Differentiable in x, weight, bias and, through the outputs, logit_scale (frozen in the reference).
    The logits are fp32, ALSO under autocast, where the reference returns 16-bit logits (its matmul runs in the autocast dtype on
    a 16-bit h and a 16-bit normalised h); here 16-bit x and weight feed the MFMA, h and everything after it stay fp32.
    PTC_PPT=0 (config.PPT_KERNELS), CPU tensors and shapes the kernel refuses (C not a multiple of 32 up to 128, D not a multiple of
    64 up to 1024, K above 256) take ppt_head_torch, as does a class embedding that requires grad; `use_kernels` overrides the first two.  return_inv_norm: also 1 / max(|h|, eps) [N]."""
    if not ppt_head_kernels(x, weight, class_embedding, use_kernels):
        return ppt_head_torch(x, weight, bias, class_embedding, logit_scale, eps, return_inv_norm)
    logits, inv = _PPTHead.apply(x, weight, bias, class_embedding.detach(), logit_scale, _ppt_scale(logit_scale), float(eps))
    return (logits, inv) if return_inv_norm else logits


def ppt_head_torch(x, weight, bias, class_embedding, logit_scale, eps: float = 0.0, return_inv_norm: bool = False):
    """the reference's expression, in the dtype (and autocast state) it is called in"""
    feat = F.linear(x, weight, bias)
    if eps == 0:
        feat_n = feat / feat.norm(dim=-1, keepdim=True)                       # v1m1 :99
    else:
        feat_n = F.normalize(feat, dim=-1, p=2, eps=eps)                      # v1m3 :120
    sim = feat_n @ class_embedding.t()
    scale = logit_scale.exp() if isinstance(logit_scale, torch.Tensor) else math.exp(float(logit_scale))
    seg_logits = scale * sim
    if return_inv_norm:
        return seg_logits, 1.0 / feat.detach().norm(dim=-1).clamp_min(eps)
    return seg_logits


# ------------------------------------------------------------------------------------------------
# SGIFormer decoder (sgiformer_v1m1_base.py, loss.py): ragged masked attention, attention-mask packing, matcher cost, targets.
# Each function runs csrc/sgiformer.hip, or its *_torch twin -- the reference's own expression, loops included -- for CPU tensors, for
# shapes the kernels refuse, and under PTC_SGI=0 (config.SGI_KERNELS).  `use_kernels` overrides the choice.
# ------------------------------------------------------------------------------------------------
def _sgi_use_kernels(t: torch.Tensor, use_kernels) -> bool:
    return bool(config.SGI_KERNELS and t.is_cuda) if use_kernels is None else bool(use_kernels)


def sgi_pack_bits(b: torch.Tensor) -> torch.Tensor:
    """bool [R, M] -> int32 words [R, ceil(M / 32)], bit c % 32 of word c / 32"""
    r, m = b.shape
    w = (m + 31) // 32
    x = torch.zeros((r, w * 32), dtype=torch.int64, device=b.device)
    x[:, :m] = b.to(torch.int64)
    x = (x.view(r, w, 32) << torch.arange(32, device=b.device)).sum(-1)
    return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)


def sgi_unpack_bits(words: torch.Tensor, m: int) -> torch.Tensor:
    """int32 words [R, ceil(M / 32)] -> bool [R, M]"""
    r = words.shape[0]
    bits = (words.to(torch.int64).unsqueeze(-1) >> torch.arange(32, device=words.device)) & 1
    return bits.reshape(r, words.shape[1] * 32)[:, :m].bool()


class SGIPacked:
    """One bit per (row, column) of the [rows_i, cols_i] blocks of a ragged batch: `words` int32, ceil(cols_i / 32) words per row, the
    rows of scene i from word off[i] (`off` int64 [S + 1] on the device).  Attention masks (set = masked out) and ground-truth
    instance masks share it."""

    def __init__(self, words, off, rows, cols):
        self.words, self.off, self.rows, self.cols = words, off, [int(r) for r in rows], [int(c) for c in cols]

    @staticmethod
    def from_bool(masks):
        rows, cols = [m.shape[0] for m in masks], [m.shape[1] for m in masks]
        dev = masks[0].device
        off, _ = ops.sgi_offsets(rows, cols, dev, True)
        words = torch.cat([sgi_pack_bits(m).reshape(-1) for m in masks]) if masks else torch.empty(0, dtype=torch.int32, device=dev)
        return SGIPacked(words, off, rows, cols)

    def to_bool(self):
        out, at = [], 0
        for r, c in zip(self.rows, self.cols):
            w = (c + 31) // 32
            out.append(sgi_unpack_bits(self.words[at:at + r * w].view(r, w), c))
            at += r * w
        return out


class _SGIAttention(Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, words, row_off, scale):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out, lse = ops.sgi_attn_fwd(q, k, v, cu_q, cu_k, words, row_off, scale)
        ctx.save_for_backward(q, k, v, out, lse, cu_q, cu_k)
        ctx.mask = (words, row_off)
        ctx.scale = scale
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, cu_q, cu_k = ctx.saved_tensors
        dq, dk, dv = ops.sgi_attn_bwd(q, k, v, out, dout, lse, cu_q, cu_k, ctx.mask[0], ctx.mask[1], ctx.scale)
        return dq, dk, dv, None, None, None, None, None


def sgi_attention(q, k, v, lq, lk, mask=None, scale=None, use_kernels=None):
    """Multi-head attention of every scene of a ragged batch in one launch: q [Tq, H, D], k, v [Tk, H, D]; scene i attends its lq[i]
    query rows to its lk[i] key rows (host lists).  mask: an SGIPacked [lq_i, lk_i] or a list of bool [lq_i, lk_i], True / set =
    masked out, shared by the heads, no row fully masked.  fp32 or bf16 rows (other dtypes are computed in fp32); bf16 MFMA operands,
    fp32 accumulation and softmax; nothing of size Lq x Lk is written to memory.  D = 32 on the kernels, other head dims on torch."""
    if not (_sgi_use_kernels(q, use_kernels) and ops.sgi_attn_supported(q.shape[-1])):
        return sgi_attention_torch(q, k, v, lq, lk, mask, scale)
    if mask is not None and not isinstance(mask, SGIPacked):
        mask = SGIPacked.from_bool(mask)
    dt = q.dtype if q.dtype in (torch.float32, torch.bfloat16) else torch.float32
    cu_q, cu_k = ops.sgi_cu(lq, q.device), ops.sgi_cu(lk, q.device)
    words, row_off = (None, None) if mask is None else (mask.words, mask.off)
    with torch.autocast(device_type=q.device.type, enabled=False):
        out = _SGIAttention.apply(q.to(dt), k.to(dt), v.to(dt), cu_q, cu_k, words, row_off, scale)
    return out.to(q.dtype)


def sgi_attention_torch(q, k, v, lq, lk, mask=None, scale=None):
    """nn.MultiheadAttention's own arithmetic (need_weights=True path: scaled q, additive -inf mask, dense softmax, bmm), one scene
    after the other as CrossAttentionLayer / SelfAttentionLayer (:208-248) loop"""
    if isinstance(mask, SGIPacked):
        mask = mask.to_bool()
    scale = float(q.shape[-1]) ** -0.5 if scale is None else float(scale)
    outs, aq, ak = [], 0, 0
    for i, (nq, nk) in enumerate(zip(lq, lk)):
        qi = (q[aq:aq + nq] * scale).transpose(0, 1)         # [H, Lq, D]
        ki, vi = k[ak:ak + nk].transpose(0, 1), v[ak:ak + nk].transpose(0, 1)
        if mask is not None:
            bias = torch.zeros(mask[i].shape, dtype=qi.dtype, device=qi.device).masked_fill_(mask[i], float("-inf"))
            attn = torch.baddbmm(bias.unsqueeze(0).expand(qi.shape[0], -1, -1), qi, ki.transpose(-2, -1))
        else:
            attn = torch.bmm(qi, ki.transpose(-2, -1))
        attn = F.softmax(attn, dim=-1)
        outs.append(torch.bmm(attn, vi).transpose(0, 1))
        aq, ak = aq + nq, ak + nk
    return torch.cat(outs, 0)


def sgi_pack_mask(logits, use_kernels=None):
    """The attention masks of forward_head (:372-378) for every scene in one launch: logits = list of [lq_i, M_i] mask logits ->
    SGIPacked with a bit set where sigmoid(x) < 0.5, rows whose bits would all be set cleared.  Not differentiable."""
    if not _sgi_use_kernels(logits[0], use_kernels):
        return SGIPacked.from_bool(sgi_pack_mask_torch(logits))
    lq, lk = [x.shape[0] for x in logits], [x.shape[1] for x in logits]
    flat = torch.cat([x.detach().float().reshape(-1) for x in logits])
    words, row_off = ops.sgi_pack_mask(flat, lq, lk)
    return SGIPacked(words, row_off, lq, lk)


def sgi_pack_mask_torch(logits):
    out = []
    for pred_mask_ in logits:
        attn_mask_ = (pred_mask_.sigmoid() < 0.5).bool()
        attn_mask_[torch.where(attn_mask_.sum(-1) == attn_mask_.shape[-1])] = False
        out.append(attn_mask_.detach())
    return out


def sgi_match_cost(mask_logits, cls_logits, gt_masks, gt_cls, weights=(0.5, 1.0, 1.0), use_kernels=None):
    """The Hungarian matcher's cost matrices of every scene of a level in one launch (loss.py:331-429):
    w_cls (-softmax(cls)[:, gt_cls]) + w_bce BCE + w_dice dice, non-finite entries replaced by 1e6.  mask_logits: list of
    [lq_i, M_i]; cls_logits: list of [lq_i, C]; gt_masks: SGIPacked [G_i, M_i] (or a list of bool); gt_cls: list of int64 [G_i].
    -> list of fp32 [lq_i, G_i].  No gradient (the reference runs it under no_grad)."""
    with torch.no_grad():
        if not _sgi_use_kernels(mask_logits[0], use_kernels):
            return sgi_match_cost_torch(mask_logits, cls_logits, gt_masks, gt_cls, weights)
        if not isinstance(gt_masks, SGIPacked):
            gt_masks = SGIPacked.from_bool(gt_masks)
        lq, lk, g = [x.shape[0] for x in mask_logits], [x.shape[1] for x in mask_logits], [int(c.numel()) for c in gt_cls]
        flat = torch.cat([x.float().reshape(-1) for x in mask_logits])
        cost, off = ops.sgi_match_cost(flat, torch.cat([c.float() for c in cls_logits]), lq, lk, g, gt_masks.words, gt_masks.off,
                                       torch.cat([c.to(torch.int64) for c in gt_cls]), weights)
        return [cost[off[i]:off[i + 1]].view(lq[i], g[i]) for i in range(len(lq))]


def sgi_match_cost_torch(mask_logits, cls_logits, gt_masks, gt_cls, weights=(0.5, 1.0, 1.0)):
    if isinstance(gt_masks, SGIPacked):
        gt_masks = gt_masks.to_bool()
    out = []
    for inputs, cls, targets, inst_cls in zip(mask_logits, cls_logits, gt_masks, gt_cls):
        inputs, targets = inputs.float(), targets.float()
        score = cls.softmax(-1)
        cost_cls = -score[:, inst_cls.long()] * weights[0]
        pos = F.binary_cross_entropy_with_logits(inputs, torch.ones_like(inputs), reduction="none")
        neg = F.binary_cross_entropy_with_logits(inputs, torch.zeros_like(inputs), reduction="none")
        pos_loss = torch.einsum("nc,mc->nm", pos, targets)
        neg_loss = torch.einsum("nc,mc->nm", neg, (1 - targets))
        cost_bce = (pos_loss + neg_loss) / inputs.shape[1] * weights[1]
        sig = inputs.sigmoid()
        numerator = 2 * torch.einsum("nc,mc->nm", sig, targets)
        denominator = sig.sum(-1)[:, None] + targets.sum(-1)[None, :]
        cost_dice = (1 - (numerator + 1) / (denominator + 1)) * weights[2]
        cost_value = torch.stack([cost_cls, cost_bce, cost_dice]).sum(dim=0)
        cost_value = torch.where(torch.isnan(cost_value) | torch.isinf(cost_value), torch.full_like(cost_value, 1e6), cost_value)
        out.append(cost_value)
    return out


class SGITargets:
    """prepare_target's instance information of a batch: counts (list of int32 [G_i, M_i]: points of instance g in superpoint m),
    masks (SGIPacked [G_i, M_i]: 2 count > superpoint size), cls (list of int64 [G_i]); G_i = max instance + 1, 0 without any."""

    def __init__(self, counts, masks, cls):
        self.counts, self.masks, self.cls = counts, masks, cls


def _sgi_scene_sizes(instance, sp_inverse, offset):
    """host (bounds, superpoints per scene, instances per scene) with ONE device -> host copy"""
    ends = offset.to(torch.int64)
    s = ends.numel()
    if instance.numel() == 0:
        return [(0, 0)] * s, [0] * s, [0] * s
    starts = torch.cat([ends.new_zeros(1), ends[:-1]])
    seg = torch.repeat_interleave(torch.arange(s, device=ends.device), ends - starts)
    imax = torch.full((s,), -1, dtype=torch.int64, device=ends.device).scatter_reduce_(0, seg, instance.to(torch.int64), "amax")
    smax = torch.full((s,), -1, dtype=torch.int64, device=ends.device).scatter_reduce_(0, seg, sp_inverse.to(torch.int64), "amax")
    smin = torch.full((s,), 2 ** 62, dtype=torch.int64, device=ends.device).scatter_reduce_(0, seg, sp_inverse.to(torch.int64), "amin")
    host = torch.stack([ends, imax, smin, smax]).tolist()
    bounds = list(zip([0] + host[0][:-1], host[0]))
    lk = [int(b - a + 1) if b >= a else 0 for a, b in zip(host[2], host[3])]
    g = [max(int(m) + 1, 0) for m in host[1]]
    return bounds, lk, g


def sgi_targets(instance, segment, sp_inverse, offset, use_kernels=None) -> SGITargets:
    """prepare_target (:538-584) for all scenes in one pass, without the [N, G] one-hot.  instance, segment (already remapped),
    sp_inverse (the global superpoint row of each point, rows grouped by scene) per point; offset [S].  Points with instance < 0
    count towards the size of their superpoint and towards nothing else (the reference's scatter-max indexes with -1 there, which the
    CUDA library leaves undefined: such rows are skipped, here and in the golden generator)."""
    with torch.no_grad():
        if not _sgi_use_kernels(instance, use_kernels):
            return sgi_targets_torch(instance, segment, sp_inverse, offset)
        _, lk, g = _sgi_scene_sizes(instance, sp_inverse, offset)
        _, counts, words, word_off, inst_cls = ops.sgi_targets(instance, segment, sp_inverse, offset, lk, g)
        cl, il, ac, ai = [], [], 0, 0
        for gi, mi in zip(g, lk):
            cl.append(counts[ac:ac + gi * mi].view(gi, mi))
            il.append(inst_cls[ai:ai + gi])
            ac, ai = ac + gi * mi, ai + gi
        return SGITargets(cl, SGIPacked(words, word_off, g, lk), il)


def sgi_targets_torch(instance, segment, sp_inverse, offset) -> SGITargets:
    ends = [int(e) for e in offset.tolist()]
    counts, masks, cls = [], [], []
    for start, end in zip([0] + ends[:-1], ends):
        instance_, segment_ = instance[start:end].long(), segment[start:end].long()
        sp_inverse_ = sp_inverse[start:end].long()
        sp_inverse_ = sp_inverse_ - sp_inverse_.min()
        m = int(sp_inverse_.max()) + 1
        if instance_.max() >= 0:
            inst_onehot_ = torch.zeros((instance_.shape[0], int(instance_.max()) + 1), device=instance_.device, dtype=instance_.dtype)
            inst_mask_ = instance_ != -1
            inst_onehot_[inst_mask_] = F.one_hot(instance_[inst_mask_], inst_onehot_.shape[1])
            count_ = torch.zeros((m, inst_onehot_.shape[1]), device=instance_.device, dtype=instance_.dtype).index_add_(0, sp_inverse_, inst_onehot_)
            size_ = torch.bincount(sp_inverse_, minlength=m)
            inst_sp_mask_ = (count_.double() / size_.clamp(min=1).unsqueeze(1)).T > 0.5
            inst_cls_ = torch.full((inst_onehot_.shape[1],), torch.iinfo(torch.int64).min, device=instance_.device, dtype=torch.int64)
            inst_cls_ = inst_cls_.scatter_reduce(0, instance_[inst_mask_], segment_[inst_mask_], "amax")
            inst_cls_[inst_cls_ == torch.iinfo(torch.int64).min] = 0
            counts.append(count_.T.to(torch.int32).contiguous())
        else:
            inst_sp_mask_ = torch.zeros((0, m), device=instance_.device, dtype=torch.bool)
            inst_cls_ = torch.zeros(0, device=instance_.device, dtype=torch.int64)
            counts.append(torch.zeros((0, m), device=instance_.device, dtype=torch.int32))
        masks.append(inst_sp_mask_)
        cls.append(inst_cls_)
    return SGITargets(counts, SGIPacked.from_bool(masks), cls)


# ------------------------------------------------------------------------------------------------
# Sonata-v1m1 (sonata_v1m1_base.py:267-291, :443-454): Sinkhorn-Knopp targets from the teacher and the soft cross entropy of the
# student against them, reduced to the mean over scenes of the per-scene means.  csrc/sonata.hip keeps the Sinkhorn matrix as two
# scaling vectors (e_ik a_k b_i) and never stores anything of size M x K; sonata_distill_torch is the reference's expression, used
# for CPU tensors, for prototype counts the kernels refuse and under PTC_SONATA=0 (config.SONATA_KERNELS).
# ------------------------------------------------------------------------------------------------
def _sonata_use_kernels(teacher_sim, student_sim, num_iter, use_kernels) -> bool:
    if use_kernels is None:
        use_kernels = config.SONATA_KERNELS and teacher_sim.is_cuda
    return bool(use_kernels and num_iter >= 1 and teacher_sim.dtype != torch.float64 and student_sim.dtype != torch.float64
                and teacher_sim.dim() == 2 and ops.sonata_supported(teacher_sim.shape[1]))


def sonata_sinkhorn_scales(teacher_sim, match_index, teacher_temp: float, num_iter: int = 3, all_reduce=None, max_groups: int = 0):
    """The prototype scales a [K] after num_iter Sinkhorn-Knopp iterations over e_ik = exp(teacher_sim[match_index[i, 1]] / temp):
    the assignment of :267-291 is e_ik a_k / sum_k e_ik a_k.  num_iter passes over the teacher rows (the last row normalisation is
    left to the loss pass).  all_reduce(tensor) sums a tensor over the ranks in place: it is called on the row count and on every
    K-vector of column sums."""
    m, k = match_index.shape[0], teacher_sim.shape[1]
    n = float(m)
    if all_reduce is not None:
        cnt = torch.tensor([m], dtype=torch.float64, device=teacher_sim.device)
        all_reduce(cnt)
        n = float(cnt.item())
    r = ops.sonata_colsum(teacher_sim, match_index, teacher_temp, None, max_groups)
    for it in range(num_iter):
        if all_reduce is not None:
            all_reduce(r)
        a = torch.reciprocal(r * float(k))
        if it + 1 < num_iter:
            _, _, r = ops.sonata_rowpass(teacher_sim, match_index, teacher_temp, a, n, True, max_groups)
    return a


class _SonataDistill(Function):
    @staticmethod
    def forward(ctx, student_sim, teacher_sim, match_index, student_batch, num_scenes, teacher_temp, student_temp, num_iter, all_reduce,
                max_groups):
        a = sonata_sinkhorn_scales(teacher_sim, match_index, teacher_temp, num_iter, all_reduce, max_groups)
        loss, _, state = ops.sonata_distill_fwd(teacher_sim, student_sim, match_index, student_batch, num_scenes, teacher_temp, student_temp, a,
                                                max_groups)
        ctx.save_for_backward(*state)
        ctx.args = (float(teacher_temp), float(student_temp), int(max_groups))
        return loss[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        tt, st, cap = ctx.args
        return (ops.sonata_distill_bwd(tuple(ctx.saved_tensors), tt, st, dloss, cap),) + (None,) * 9


def sonata_distill(teacher_sim, student_sim, match_index, student_batch, teacher_temp: float, student_temp: float, num_iter: int = 3,
                   all_reduce=None, num_scenes: Optional[int] = None, max_groups: int = 0, use_kernels=None):
    """mean over scenes of the per-scene mean of -sum_k sinkhorn_knopp(teacher_sim[match_index[:, 1]], teacher_temp)_k
    log_softmax(student_sim[match_index[:, 0]] / student_temp)_k (:437-454): an fp32 scalar, differentiable in student_sim (the
    gradient has student_sim's dtype; unmatched rows are exactly zero), the teacher detached.  The scene of a pair is
    student_batch[match_index[:, 0]] and must ascend along match_index, as segment_coo requires; the divisor is the scene of the last
    pair + 1.  num_scenes bounds student_batch (default: read from its last element, one host read).  all_reduce: see
    sonata_sinkhorn_scales.  Logits in fp32, bf16 or fp16 are read as they are; all arithmetic is fp32."""
    if not _sonata_use_kernels(teacher_sim, student_sim, num_iter, use_kernels):
        return sonata_distill_torch(teacher_sim, student_sim, match_index, student_batch, teacher_temp, student_temp, num_iter, all_reduce)
    if match_index.shape[0] == 0:
        # no kernel to launch: the reference's mean over no rows (NaN) with an all-zero gradient; the other ranks still get this
        # rank's (zero) share of their column sums
        if all_reduce is not None:
            sonata_sinkhorn_scales(teacher_sim, match_index, teacher_temp, num_iter, all_reduce, max_groups)
        return student_sim[match_index[:, 0]].float().mean()
    if num_scenes is None:
        num_scenes = int(student_batch[-1]) + 1
    with torch.autocast(device_type=student_sim.device.type, enabled=False):
        return _SonataDistill.apply(student_sim, teacher_sim.detach(), match_index, student_batch, int(num_scenes), float(teacher_temp),
                                    float(student_temp), int(num_iter), all_reduce, int(max_groups))


def sonata_sinkhorn_torch(feat, temp: float, num_iter: int = 3, all_reduce=None):
    """sinkhorn_knopp (:267-291) on the gathered teacher rows feat [M, K]: fp32 (float64 input stays float64)"""
    feat = feat if feat.dtype == torch.float64 else feat.float()
    q = torch.exp(feat / temp).t()
    k = q.shape[0]
    n = q.shape[1]
    if all_reduce is not None:
        cnt = torch.tensor([n], dtype=torch.float64, device=feat.device)
        all_reduce(cnt)
        n = float(cnt.item())
    sum_q = q.sum()
    if all_reduce is not None:
        all_reduce(sum_q)
    q = q / sum_q
    for _ in range(num_iter):
        q_row_sum = q.sum(dim=1, keepdim=True)
        if all_reduce is not None:
            all_reduce(q_row_sum)
        q = q / q_row_sum / k
        q = q / q.sum(dim=0, keepdim=True) / n
    q = q * n
    return q.t()


def sonata_distill_torch(teacher_sim, student_sim, match_index, student_batch, teacher_temp: float, student_temp: float, num_iter: int = 3,
                         all_reduce=None):
    """the reference's expression (:437-454): the dense Sinkhorn matrix, log_softmax of the gathered student rows, their product,
    and segment_coo(reduce="mean") without dim_size followed by .mean()"""
    with torch.no_grad():
        target = sonata_sinkhorn_torch(teacher_sim.detach()[match_index[:, 1]], teacher_temp, num_iter, all_reduce)
    loss = -torch.sum(target * F.log_softmax(student_sim[match_index[:, 0]] / student_temp, dim=-1), dim=-1)
    if loss.shape[0] == 0:
        return loss.mean()
    index = student_batch[match_index[:, 0]].long()
    scenes = int(index[-1]) + 1
    total = torch.zeros(scenes, dtype=loss.dtype, device=loss.device).index_add(0, index, loss)
    count = torch.bincount(index, minlength=scenes).clamp(min=1)
    return (total / count).mean()


# ------------------------------------------------------------------------------------------------
# Concerto-v1m1's 2D-3D alignment branch (concerto_v1m1_base.py:528-573, :745-866) on csrc/concerto.hip: the pooled
# correspondence, the patch binning, the patch means of the 3D features and the centred cosine loss.  Each X_torch holds the
# reference's expression, used for CPU tensors and under PTC_CONCERTO=0 (config.CONCERTO_KERNELS).
# ------------------------------------------------------------------------------------------------
def _concerto_use_kernels(t: torch.Tensor, use_kernels) -> bool:
    if use_kernels is None:
        use_kernels = config.CONCERTO_KERNELS and t.is_cuda
    return bool(use_kernels)


def _segment_sum_sorted(src: torch.Tensor, idx_ptr: torch.Tensor) -> torch.Tensor:
    """torch_scatter.segment_csr(src, idx_ptr, reduce="sum") over dim 0"""
    m = idx_ptr.numel() - 1
    seg = torch.repeat_interleave(torch.arange(m, device=src.device), idx_ptr[1:] - idx_ptr[:-1])
    return torch.zeros((m,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device).index_add_(0, seg, src[: seg.numel()])


def concerto_pool_corr_torch(corr: torch.Tensor, perm: Optional[torch.Tensor], idx_ptr: torch.Tensor) -> torch.Tensor:
    """one level of pool_corr (:545-570) as the reference writes it, all images at once: the mask of the fully valid members summed
    per cluster, the -1 entries zeroed one by one, the member sum divided by the count and (-1, -1) where the count is 0"""
    m = idx_ptr.numel() - 1
    if corr.shape[1] == 0:
        return -torch.ones((m, 0, 2), device=corr.device)
    indices = perm if perm is not None else torch.arange(corr.shape[0], device=corr.device)
    ft = corr.dtype if corr.dtype == torch.float64 else torch.float32
    mask = torch.all(corr != -1, dim=2).to(ft)
    counts = _segment_sum_sorted(mask[indices], idx_ptr)
    empty = counts == 0
    counts = counts.masked_fill(empty, 100000)
    filled = corr.clone()
    filled[filled == -1] = 0
    total = _segment_sum_sorted(filled[indices], idx_ptr)
    out = total / counts.unsqueeze(-1)
    out[empty] = -1
    return out


def concerto_pool_corr(corr: torch.Tensor, perm: Optional[torch.Tensor], idx_ptr: torch.Tensor, use_kernels=None) -> torch.Tensor:
    """The point-to-pixel correspondences [N, V, 2] pooled to the M clusters of one level (perm = points sorted by cluster, idx_ptr
    [M + 1]) -> [M, V, 2] fp32; see ops.concerto_pool_corr.  No gradient."""
    if not _concerto_use_kernels(corr, use_kernels) or corr.dtype not in (torch.float32, torch.int32, torch.int64):
        return concerto_pool_corr_torch(corr, perm, idx_ptr)
    return ops.concerto_pool_corr(corr.detach(), perm, idx_ptr)


def concerto_patch_pairs_torch(corr, scene, img_offset, img_num, total_images: int, patch_h: int, patch_w: int, rows=None):
    """the patch binning of :786-830 in torch: valid pairs by torch.where (ascending point row, then view), their keys, torch.unique.
    Pairs outside their image or their scene's images are left out, as in ops.concerto_patch_pairs."""
    dev = corr.device
    sel = corr if rows is None else corr[rows]
    ns, v = sel.shape[0], sel.shape[1]
    scene = scene.long()
    r, c = sel[..., 0].long(), sel[..., 1].long()              # .long() truncates toward zero
    view = torch.arange(v, device=dev)
    # trunc(a) in [0, patch_h) <=> -1 < a < patch_h, on the values themselves: a NaN is outside (its .long() depends on the device)
    inside = (sel[..., 0] > -1) & (sel[..., 0] < patch_h) & (sel[..., 1] > -1) & (sel[..., 1] < patch_w)
    mask = torch.any(sel != -1, dim=2) & inside & (view[None] < img_num.long()[scene][:, None])
    pi, vi = torch.where(mask)
    keys = (img_offset.long()[scene[pi]] + vi) * patch_h * patch_w + r[pi, vi] * patch_w + c[pi, vi]
    ids, inv, counts = torch.unique(keys, return_inverse=True, return_counts=True)
    order = torch.argsort(inv, stable=True)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)])
    point = pi[order]
    pair_patch = torch.full((ns, v), -1, dtype=torch.int64, device=dev)
    pair_patch[pi, vi] = inv
    return ops.ConcertoPairs(ids, indptr, point if rows is None else rows.long()[point], pair_patch, None if rows is None else rows.long())


def concerto_patch_pairs(corr, scene, img_offset, img_num, total_images: int, patch_h: int, patch_w: int, rows=None, use_kernels=None):
    """ops.ConcertoPairs of the (point, image) pairs of the selected rows of the pooled correspondence; see ops.concerto_patch_pairs
    (and there for the one difference from the reference: pairs outside their image are left out)."""
    if not _concerto_use_kernels(corr, use_kernels) or corr.dtype != torch.float32:
        return concerto_patch_pairs_torch(corr, scene, img_offset, img_num, total_images, patch_h, patch_w, rows)
    return ops.concerto_patch_pairs(corr, scene, img_offset, img_num, total_images, patch_h, patch_w, rows)


class _ConcertoPatchMean(Function):
    @staticmethod
    def forward(ctx, feat, pairs):
        out, _ = ops.segment_csr_fwd(feat, pairs.perm, pairs.indptr, "mean")
        ctx.pairs, ctx.n = pairs, feat.shape[0]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return ops.concerto_patch_mean_bwd(grad, ctx.pairs, ctx.n), None


def concerto_patch_mean_torch(feat: torch.Tensor, pairs) -> torch.Tensor:
    """scatter_mean(feature3d[valid_index[0]], feature_index)[unique ids] (:826-832), compact: the rows without a pair are not made"""
    u = pairs.num_patches
    counts = pairs.indptr[1:] - pairs.indptr[:-1]
    seg = torch.repeat_interleave(torch.arange(u, device=feat.device), counts)
    total = torch.zeros((u, feat.shape[1]), dtype=feat.dtype, device=feat.device).index_add(0, seg, feat[pairs.perm])
    return total / counts.clamp(min=1).to(feat.dtype).unsqueeze(-1)


def concerto_patch_mean(feat: torch.Tensor, pairs, use_kernels=None) -> torch.Tensor:
    """mean3d [U, C]: row u = the mean of feat[p] over the pairs of patch u (the fused-gather CSR reduce of csrc/rows.hip); the
    backward gathers through pairs.pair_patch: d feat[p] = sum over p's pairs of d mean3d[u] / count[u], no atomics."""
    if not _concerto_use_kernels(feat, use_kernels) or feat.dtype == torch.float64 or pairs.num_patches == 0:
        return concerto_patch_mean_torch(feat, pairs)
    return _ConcertoPatchMean.apply(feat, pairs)


class _ConcertoAlign(Function):
    @staticmethod
    def forward(ctx, y, feature2d, patch_ids, cos_shift, eps):
        loss, _, dy = ops.concerto_align(feature2d, patch_ids, y, cos_shift, eps, ctx.needs_input_grad[0])
        ctx.save_for_backward(dy)
        return loss[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        dy, = ctx.saved_tensors
        return dy.mul_(dloss.to(torch.float32)), None, None, None, None


def concerto_align_loss_torch(feature2d, patch_ids, y, cos_shift: bool = True, eps: float = 1e-6):
    """the reference's expression (:831-842): both gathers, the centring and CosineSimilarity(dim=1, eps)"""
    x = feature2d[patch_ids]
    if cos_shift:
        x = x - x.mean(dim=-1, keepdim=True)
        y = y - y.mean(dim=-1, keepdim=True)
    return (1 - torch.nn.CosineSimilarity(dim=1, eps=eps)(x, y)).mean() * 10


def concerto_align_loss(feature2d, patch_ids, y, cos_shift: bool = True, eps: float = 1e-6, use_kernels=None):
    """10 * mean_u (1 - cos(feature2d[patch_ids[u]], y[u])), both rows centred over the channels when cos_shift: an fp32 scalar,
    differentiable in y (the gradient has y's dtype), feature2d read through the index and never copied.  The cosine is ATen's:
    each norm clamped at eps on its own, the clamp passing the gradient from eps upwards.  No patches: the reference's mean over
    nothing (NaN), without a launch."""
    if (not _concerto_use_kernels(y, use_kernels) or y.dtype == torch.float64 or feature2d.dtype == torch.float64 or y.dim() != 2
            or patch_ids.numel() == 0 or not ops.concerto_align_supported(y.shape[1])):
        return concerto_align_loss_torch(feature2d, patch_ids, y, cos_shift, eps)
    with torch.autocast(device_type=y.device.type, enabled=False):
        return _ConcertoAlign.apply(y, feature2d.detach(), patch_ids, bool(cos_shift), float(eps))
