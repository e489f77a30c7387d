"""-m gpu: nothing the Block executor (csrc/block_exec.hip) enqueues writes past the end of a slab.  The library lays the five
slabs of a Block call out itself (ptc_ptv3_block_layout) and functional._BlockFn allocates exactly the totals it is told, so a kernel
that wrote one row too many, or a slot the layout sized too small at the end of a slab, would land in a neighbour's memory.  Here every
slab gets 256 bytes more than asked, filled with 0xA5; after one forward and backward the tails must be as they were.  The tails
are only read.  The same body runs on the host emulation in tests/test_block_layout_cpu.py."""
import numpy as np
import pytest
import torch

# (points per scene, channels, heads, patch, dtype of the stream, DropPath row scales, block tables)
CASES = [(700, 32, 2, 128, torch.float32, True, False),        # fused MLP, fp32 stream: dx0 in the fp32 scratch slab
         (2300, 64, 4, 128, torch.bfloat16, False, True),       # fused MLP, 16-bit stream, block-staged convolution (conv7)
         (1500, 128, 8, 128, torch.float32, True, True)]        # ~3000 rows in two scenes: split MLP (H / ACT / M / DH exist), conv8's workspace
TAIL, FILL = 256, 0xA5


def block_call_leaves_slab_tails_intact(device, monkeypatch, n_pts, C, H, patch, a_dtype, with_rs, blk_tables):
    from oracle import maps as omaps
    from oracle import sfc as osfc
    from pointcept_amd import _lib
    from pointcept_amd import functional as PF
    from pointcept_amd import ops, synthetic

    b = synthetic.indoor_batch(2, n_pts)
    bt, gc = omaps.offset2batch(b["offset"]), b["grid_coord"]
    o = np.argsort(osfc.encode_c(gc, bt, int(gc.max() + 1).bit_length(), ("hilbert",))[0], kind="stable")
    ind = torch.from_numpy(np.concatenate([bt[o, None], gc[o]], 1).astype(np.int32)).to(device)
    n = ind.shape[0]
    g = torch.Generator().manual_seed(C)

    def P(*s, scale=1.0, shift=0.0):
        return (shift + torch.randn(*s, generator=g) * scale).to(device).requires_grad_(True)

    params = [P(C, 3, 3, 3, C, scale=(27 * C) ** -0.5), P(C, scale=0.1), P(C, C, scale=C ** -0.5), P(C, scale=0.1), P(C, scale=0.1, shift=1.0),
              P(C, scale=0.1), P(C, scale=0.1, shift=1.0), P(C, scale=0.1), P(3 * C, C, scale=C ** -0.5), P(3 * C, scale=0.1),
              P(C, C, scale=C ** -0.5), P(C, scale=0.1), P(C, scale=0.1, shift=1.0), P(C, scale=0.1), P(4 * C, C, scale=C ** -0.5),
              P(4 * C, scale=0.1), P(C, 4 * C, scale=(4 * C) ** -0.5), P(C, scale=0.1)]
    x0 = torch.randn(n, C, generator=g).to(a_dtype).to(device).requires_grad_(True)
    xc = torch.randn(n, C, generator=g).to(torch.bfloat16).to(device).requires_grad_(True)
    nbr = ops.rulebook_subm(ind, 3)
    offs = torch.from_numpy(b["offset"].astype(np.int64))
    key = torch.from_numpy(bt[o].astype(np.int64)) * 10 ** 9 + torch.from_numpy(np.random.default_rng(2).integers(0, 10 ** 8, n))
    order = torch.argsort(key)                                  # some serialization order that keeps the scenes contiguous
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(n)
    pad, unpad, cu, dup = ops.patch_pad_maps(offs.to(device), [int(v) for v in offs], patch)
    tabs = ops.attn_tables(order.to(device), inverse.to(device), pad, unpad, dup)
    blk = ops.BlockTables(nbr) if blk_tables else None
    rs1 = ((torch.rand(n, generator=g) > 0.3).float() / 0.7).to(device) if with_rs else None
    rs2 = ((torch.rand(n, generator=g) > 0.3).float() / 0.7).to(device) if with_rs else None
    meta = dict(dt=torch.bfloat16, n_pad=int(tabs[0].shape[1]), n_seq=int(cu.numel()) - 1, heads=H, patch=patch, scale=16 ** -0.5, eps_cpe=1e-5,
                eps_n1=1e-5, eps_n2=1e-5, nbr=nbr, blk=blk, tabs=tabs, cu=cu)
    dz, dyb = torch.randn(n, C, generator=g).to(device), torch.randn(n, C, generator=g).to(torch.bfloat16).to(device)

    slabs, real = [], PF._blk_alloc

    def padded(nbytes, dtype, dev):
        t = real(nbytes + TAIL, dtype, dev)
        t.view(torch.uint8)[nbytes:] = FILL
        slabs.append((t, nbytes))
        return t

    monkeypatch.setattr(PF, "_blk_alloc", padded)
    x3, xb = PF.ptv3_block(x0, xc, rs1, rs2, meta, params)
    torch.autograd.backward([x3, xb], [dz, dyb])
    if device.type == "cuda":
        torch.cuda.synchronize()
    # the five slabs, of the sizes the library's layout names for this shape: two in the forward, three in the backward
    E = _lib.block_enums()
    plan = PF._blk_plans[(n, meta["n_pad"], C, H, a_dtype, torch.bfloat16)]
    assert [nb for _, nb in slabs] == [plan["bytes"][E["SLAB_" + k]] for k in ("SAVED16", "SAVED32", "PGRAD", "SCRATCH32", "SCRATCH16")]
    for k, (t, nbytes) in zip(("saved16", "saved32", "param_grad", "scratch32", "scratch16"), slabs):
        tail = t.view(torch.uint8)[nbytes:]
        assert tail.numel() == TAIL and bool((tail == FILL).all()), f"slab {k} ({nbytes} bytes): bytes past its end were written"
    # the call did run: finite outputs and gradients for both inputs and every parameter
    for t in [x3, xb, x0.grad, xc.grad] + [p.grad for p in params]:
        assert t is not None and bool(torch.isfinite(t.float()).all())
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"c{c[1]}" for c in CASES])
def test_block_executor_writes_nothing_past_a_slab(cuda, monkeypatch, case):
    from pointcept_amd import functional as PF

    PF.invalidate_weight_casts()
    try:
        block_call_leaves_slab_tails_intact(cuda, monkeypatch, *case)
    finally:
        PF.invalidate_weight_casts()
