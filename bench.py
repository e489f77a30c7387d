#!/usr/bin/env python
"""bench.py -- BASELINE.json metric on MI355X: scenes/sec of one training step (forward + backward
+ optimizer) of DefaultSegmentorV2(PT-v3m1) on ScanNet-shaped synthetic scenes.

    python bench.py --gpus N --steps K --warmup W            (N > 1: spawns its own N ranks, see below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Workload (BASELINE.json configs[2] / SURVEY 8(d) config 3): PT-v3m1 base (46,166,272 parameters,
4 serialization orders, patch 1024), batch 8 scenes x 102,400 voxels PER GPU (weak scaling),
16-bit autocast (`--amp bf16` default; `--amp fp16` = the reference's recipe: fp16 autocast +
torch.amp.GradScaler, engines/train.py:203-231), criteria CrossEntropy + Lovasz-Softmax as in
configs/scannet/semseg-pt-v3m1-0-base.py:48-52 (`--ce-only` drops the Lovasz term), AdamW.
N > 1: one process per GPU, DistributedDataParallel over RCCL through pointcept_amd/dp.py
(gradient all-reduce overlapped with backward).  Started WITHOUT a torchrun environment and with
--gpus N > 1, this file launches its own N workers (the role of pointcept/engines/launch.py:106-136)
and refuses to report anything but n_gpus = N.
Inputs are generated on the host, copied to HBM BEFORE the timed region and reused every step
(rulebooks, sort, pad maps are rebuilt every step -- nothing is cached across steps).

Prints ONE JSON line on rank 0 (contract of the driver).  A plain run does only what that line's headline needs: it sets up,
warms up, times --steps steps, writes --dump-outputs if asked and prints metric / value / unit / ms_per_step / dtype / config.
--full adds, after the timed steps (none of it changes the headline or the dumped arrays):
  step_traffic    : HBM bytes of one step, read from the latest committed profiles/*_step_traffic.txt (not measured here)
  roofline        : the dominant kernel (serialized attention forward at the dec0/enc0 shapes),
                    timed live with HIP events on the launch stream
  roofline_gather : the gather-table convolution (CPE conv 64->64 at stage 0), HBM-bound by SURVEY 8(d)
  roofline_gemm   : the Linear layers of a stage-3 Block (256 channels, ~20000 rows: qkv, fc1 + GELU, fc2 and the five weight gradients),
                    MFMA-bound by SURVEY 8(d): gemm3.h / wgrad3.h against the bf16 matrix peak
  secondary       : BASELINE configs[1] (SpUNet-v1m1, 8 x 100000 voxels) measured in the same process, with its fp16 recipe;
                    secondary_outdoor (configs[4]) and secondary_f2 (PT-v3m2 at the Sonata widths) after it
  recipe_fp16     : the headline step under fp16 autocast + GradScaler, measured by a child process
  cpu_baseline    : the CPU oracle (oracle/ptv3_model.py, port of the reference model) timed on this
                    box's host cores on a bounded sample (rank 0, N=1 only)
  per_rank_ms_per_step, ms_per_step_without_gradient_exchange : N > 1 only, every rank's own step time and the step without DDP's all-reduce
(--no-secondary, --no-cpu-baseline and --no-fp16-recipe drop parts of that set.)

--dump-outputs DIR writes what the last timed step computed (loss, logits, gradients, updated parameters; fixed seeded
samples of the large ones) as DIR/*.npy, so that two builds run with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
PTV3_BASE = dict(  # configs/scannet/semseg-pt-v3m1-0-base.py:15-47
    in_channels=6, order=ORDERS, stride=(2, 2, 2, 2), enc_depths=(2, 2, 2, 6, 2), enc_channels=(32, 64, 128, 256, 512),
    enc_num_head=(2, 4, 8, 16, 32), enc_patch_size=(1024,) * 5, dec_depths=(2, 2, 2, 2), dec_channels=(64, 64, 128, 256),
    dec_num_head=(4, 4, 8, 16), dec_patch_size=(1024,) * 4, mlp_ratio=4, qkv_bias=True, drop_path=0.3,
    shuffle_orders=True, pre_norm=True, enable_flash=True, upcast_attention=False, upcast_softmax=False)
SPUNET_BASE = dict(channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2))  # scannet/semseg-spunet-v1m1-0-base.py:16-17

MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA peak, MI355X_MICROARCH.md "Chip-level parameters"
HBM_PEAK_GBPS = 8000.0          # HBM3E spec peak, same table (6.29 TB/s is what a float4 copy reaches)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8, help="scenes per GPU")
    ap.add_argument("--points", type=int, default=102400, help="voxels per scene")
    ap.add_argument("--full", action="store_true",
                    help="after the headline steps, also measure the rooflines, the secondary workloads, the fp16 recipe, the CPU baseline and "
                         "the multi-GPU diagnostics (a plain run measures the headline only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the SpUNet (configs[1]) measurement and the gather roofline")
    ap.add_argument("--ce-only", action="store_true", help="criteria = CrossEntropy only (default: CE + Lovasz-Softmax, the config's criteria)")
    ap.add_argument("--lovasz", action="store_true", help="(kept for old command lines; CE + Lovasz is the default)")
    ap.add_argument("--amp", default="bf16", choices=["bf16", "fp16"],
                    help="autocast dtype; fp16 adds torch.amp.GradScaler exactly as engines/train.py:203-231")
    ap.add_argument("--model", default="ptv3", choices=["ptv3", "spunet", "ptv3-outdoor", "ptv3m2-sonata"],
                    help="ptv3 = BASELINE.json metric (configs[2]); spunet = configs[1] (SpUNet-v1m1, 100000 voxels/scene); ptv3-outdoor = "
                         "configs[4] (LiDAR sweeps, depth-12 grid) as the main model (profiling); each reported with its own metric name")
    ap.add_argument("--cpu-sample-points", type=int, default=10240)
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--no-fp16-recipe", action="store_true",
                    help="skip the extra measurement of the same step under the reference's fp16 autocast + GradScaler recipe")
    ap.add_argument("--stub", action="store_true",
                    help="launcher / DP plumbing check without a GPU: gloo backend, CPU tensors, a small torch model "
                         "(tests/test_dp_gloo.py); never a benchmark result")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (rank 0; see dump_outputs)")
    return ap.parse_args(argv)


# ----------------------------------------------------------------------------------------------------------------
# self-launch (pointcept/engines/launch.py:106-136 spawns one worker per GPU; here: re-exec under torch.distributed.run)
# ----------------------------------------------------------------------------------------------------------------
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args) -> int:
    """--gpus N > 1 without a torchrun environment: start N ranks of this file on this node, one per GPU."""
    if not args.stub:
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: this node exposes {have} GPU(s); refusing to run fewer ranks than asked")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


# ----------------------------------------------------------------------------------------------------------------
# rooflines of the two dominant kernels, timed live
# ----------------------------------------------------------------------------------------------------------------
def _time_launches(fn, iters=40, warm=25):
    # 25 untimed launches first: in an otherwise idle process the first few launches of a ~0.5 ms kernel run below the clock the
    # part sustains under it (the same kernel measured 548 us as the first timing of a process and 476 us later in the same process,
    # profiles/r02_h_attn_variants.txt; rocprofv3 averages 455-470 us) -- the HIP-event average must describe the steady state
    for _ in range(warm):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()   # torch's current stream IS the stream ops.* launch on (_lib.stream_ptr)
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def _latest_profile(pattern):
    # session tags run r01_a .. r01_z, r01_aa .., r02_a ..: order by (round, length, name)
    fs = glob.glob(os.path.join(ROOT, "profiles", pattern))
    return sorted(fs, key=lambda q: (os.path.basename(q)[:3], len(os.path.basename(q)), os.path.basename(q)))[-1] if fs else None


def step_traffic():
    """HBM bytes of ONE steady-state step of this workload, from the round's committed PMC table: the TOTAL line of the
    latest profiles/*_step_traffic.txt -- FETCH_SIZE x 2 (the guide's gfx950 correction) + WRITE_SIZE over separate --pmc passes of
    `bench.py --steps 2 | 5` (tools/gpu_session.sh traffic, tools/step_traffic.py).  Not re-measured inside the timed run (counters need
    rocprofv3 around the process); the source file is named beside the number."""
    import re

    f = _latest_profile("*_step_traffic.txt")
    if not f:
        return None
    for line in open(f):
        m = re.match(r"TOTAL\s+read\s+([0-9.]+) GB\s+written\s+([0-9.]+) GB\s+sum\s+([0-9.]+) GB", line)
        if m:
            return {"step_traffic_gb": float(m.group(3)), "read_gb": float(m.group(1)), "written_gb": float(m.group(2)),
                    "compulsory_gb": 24.0, "source": os.path.relpath(f, ROOT)}
    return None


def attention_roofline(device, scenes: int, points: int):
    """Time attn_fwd_kernel alone at the shape of the largest attention of the model (dec0:
    C=64 -> H=4, N' = scenes*points padded to patches of 1024) with HIP events on the launch
    stream.  Algorithmic flops per launch = 4 L^2 D per (sequence, head)."""
    from pointcept_amd import ops

    L, H, D = 1024, 4, 16
    n_seq = scenes * ((points + L - 1) // L)
    T = n_seq * L
    g = torch.Generator(device="cpu").manual_seed(0)
    qkv = torch.randn(T, 3, H, D, generator=g).to(torch.bfloat16).to(device)
    cu = torch.arange(0, T + 1, L, dtype=torch.int32, device=device)
    scale = D ** -0.5
    ms = _time_launches(lambda: ops.attn_varlen_fwd(qkv, cu, L, scale))
    flops = 4.0 * L * L * D * n_seq * H
    achieved = flops / (ms * 1e-3) / 1e12
    out = {"kernel": "attn_fwd_kernel", "bound": "mfma", "achieved": round(achieved, 2), "peak": MFMA_BF16_PEAK_TFLOPS,
           "unit": "TFLOP/s", "frac": round(achieved / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None,
           "launch_ms": round(ms, 4), "shape": {"n_seq": n_seq, "L": L, "H": H, "D": D},
           "algorithmic_flops_per_launch": flops, "algorithmic_bytes_per_launch": T * H * D * 2 * 4}
    # the backward at the same shape (side key; SURVEY 8(d): 10 L^2 D per (sequence, head) with recomputation -- the one-pass kernel of
    # csrc/attention_bwd1.h evaluates S' / dP once and issues 8 L^2 D; priced at 8(d)'s figure all the same)
    try:
        o, lse = ops.attn_varlen_fwd(qkv, cu, L, scale)
        do = torch.randn(T, H, D, generator=g).to(torch.bfloat16).to(device)
        ms_b = _time_launches(lambda: ops.attn_varlen_bwd(qkv, o, do, lse, cu, L, scale), iters=20, warm=10)
        fb = 10.0 * L * L * D * n_seq * H
        out["backward"] = {"kernel": "attn_bwd1_kernel", "launch_ms": round(ms_b, 4), "achieved": round(fb / (ms_b * 1e-3) / 1e12, 2),
                           "frac": round(fb / (ms_b * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4), "algorithmic_flops_per_launch": fb,
                           "algorithmic_bytes_per_launch": T * H * D * 2 * 8}
    except Exception as e:   # the side key must not take the roofline object with it
        out["backward"] = {"error": repr(e)}
    # HBM bytes per launch of this kernel at this shape, from the committed rocprofv3 PMC passes (FETCH_SIZE x 2 on
    # gfx950 + WRITE_SIZE, separate --pmc runs: tools/gpu_session.sh roof); not re-measured inside bench.py
    try:
        pm = _latest_profile("*attn_pmc.json")
        ks = json.load(open(pm))["kernels"]
        k = ks[sorted(n for n in ks if n.startswith("attn_fwd_kernel"))[0]]    # r02 files carry the template arguments
        if (n_seq, H) == (800, 4):
            out["traffic"] = round(k["hbm_bytes"])
            out["traffic_source"] = os.path.relpath(pm, ROOT)
            out["mfma_busy_frac"] = round(k["SQ_VALU_MFMA_BUSY_CYCLES_mean"] * 32 / (k["GRBM_GUI_ACTIVE_mean"] * 1024), 3)
            # what actually bounds the kernel, from the same committed PMC passes: instruction issue and the vector
            # pipe, at the shader clock the part sustains under this kernel (GRBM_GUI_ACTIVE cycles per microsecond)
            g = k["GRBM_GUI_ACTIVE_mean"]
            out["valu_busy_frac"] = round(k["SQ_ACTIVE_INST_VALU_mean"] * 4 / (g * 32), 3)
            out["inst_issue_busy_frac"] = round(k["SQ_ACTIVE_INST_ANY_mean"] * 4 / (g * 32), 3)
            out["shader_clock_ghz_under_kernel"] = round(g / k["avg_us"] / 1e3, 2)
            out["bound_note"] = ("head_dim 16: one v_exp per 64 MFMA flops; the kernel is instruction-issue / VALU bound (see *_busy_frac), "
                                 "the MFMA peak is the nominal roof SURVEY 8(d) asks for")
    except Exception:
        pass
    return out


def gather_roofline(device, batch):
    """The gather-table convolution at its largest shape in the model: the CPE convolution of dec0 (SubM k=3,
    64 -> 64 channels, N = all voxels of the batch, rows in curve order as the model keeps them).  HBM-bound by
    SURVEY 8(d): algorithmic bytes = N C e (in) + N C e (out) + 8 B per (in, out) pair of the rulebook + kv C C e (weights) -- the
    pair-list formula; achieved = those bytes / launch time (the bytes of the block-local tables the kernel really reads are
    reported beside it).  `wide` (round 6): the same rulebook at 128 -> 96 channels on conv8, priced against the MFMA peak."""
    from pointcept_amd import ops

    gc, off = batch["grid_coord"], batch["offset"]
    n = gc.shape[0]
    counts = torch.diff(off, prepend=off.new_zeros(1))
    b = torch.repeat_interleave(torch.arange(off.shape[0], device=device), counts)
    depth = int(gc.max().item()).bit_length()
    code = ops.serialize_encode(gc, b, depth, ("hilbert",))
    order, _ = ops.sort_keys(code, 0, 3 * depth + max(1, (off.shape[0] - 1).bit_length()))
    ind = torch.cat([b[:, None].int(), gc.int()], 1)[order[0]].contiguous()
    nbr = ops.rulebook_subm(ind, 3, ops.HashTable(ind))
    pairs = int((nbr >= 0).sum())
    c, kv = 64, 27
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(n, c, generator=g).to(torch.bfloat16).to(device)
    w = (torch.randn(c, kv, c, generator=g) * 0.05).to(torch.bfloat16).to(device)
    bias = torch.zeros(c, device=device)
    blk = ops.BlockTables(nbr)       # the block-local tables the model builds once per rulebook (conv7: weights in registers, halo rows by DMA)
    ms = _time_launches(lambda: ops.spconv_fwd(x, w, bias, nbr, blk))
    ms_global = _time_launches(lambda: ops.spconv_fwd(x, w, bias, nbr), iters=10, warm=5)   # conv5, the round-2 kernel, for the record
    # algorithmic bytes = N C e (in) + N C e (out) + 8 B per (in, out) pair + kv C C e (weights) -- the pair-list formula
    # is what `achieved` / `frac` are quoted on.  What this kernel actually READS as its table is the block-local
    # uint16 one of ITS channel variant (tab[0]: 28 * 2 B per row) + the halo lists of the blocks that fit: reported beside it.
    nbytes_pairs = n * c * 2 * 2 + 8 * pairs + kv * c * c * 2
    nbytes_blk = n * c * 2 * 2 + blk.tab[0].numel() * 2 + int(blk.hcnt.clamp_min(0).sum().item()) * 4 + kv * c * c * 2
    flops = 2.0 * pairs * c * c
    achieved = nbytes_pairs / (ms * 1e-3) / 1e9
    out = {"kernel": "conv7_kernel (SubM k=3, 64->64, stage 0; conv5_kernel in round 2)", "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS,
           "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": None, "launch_ms": round(ms, 4),
           "shape": {"n": n, "c_in": c, "c_out": c, "kv": kv, "pairs": pairs, "halo_rows_per_128_row_block": round(float(blk.hcnt.float().mean()), 1)},
           "algorithmic_bytes_per_launch": nbytes_pairs, "algorithmic_flops_per_launch": flops,
           "bytes_with_block_tables_instead_of_pair_list": nbytes_blk,
           "frac_with_block_tables": round(nbytes_blk / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
           "global_gather_kernel_launch_ms": round(ms_global, 4),
           "useful_tflops": round(flops / (ms * 1e-3) / 1e12, 1)}
    # round 6: the same rulebook at SpUNet's widest level-0 shape (decoder block: 128 -> 96) on conv8, the block-staged kernel for rows of
    # 96 channels and more -- MFMA-bound by SURVEY 8(d) (2 x pairs x c_in x c_out useful flops); conv3's global gathers beside it
    try:
        ci, co = 128, 96
        xw = torch.randn(n, ci, generator=g).to(torch.bfloat16).to(device)
        ww = (torch.randn(co, kv, ci, generator=g) * 0.03).to(torch.bfloat16).to(device)
        bw = torch.zeros(co, device=device)
        ms_w = _time_launches(lambda: ops.spconv_fwd(xw, ww, bw, nbr, blk), iters=10, warm=3)
        ms_w3 = _time_launches(lambda: ops.spconv_fwd(xw, ww, bw, nbr), iters=5, warm=2)
        fl = 2.0 * pairs * ci * co
        out["wide"] = {"kernel": "conv8_kernel (SubM k=3, 128->96, SpUNet decoder level 0) + its conv3 follow-up for blocks whose halo does not fit",
                       "bound": "mfma", "achieved": round(fl / (ms_w * 1e-3) / 1e12, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                       "frac": round(fl / (ms_w * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4), "launch_ms": round(ms_w, 4),
                       "algorithmic_flops_per_launch": fl, "global_gather_kernel_launch_ms": round(ms_w3, 4),
                       "blocks_beyond_the_lds_image": int(((blk.hcnt < 0) | (blk.hcnt > 416)).sum().item()), "blocks": int(blk.hcnt.numel())}
        del xw, ww
    except Exception as e:       # (never takes the headline down)
        out["wide"] = {"error": repr(e)[:200]}
    try:
        pm = _latest_profile("*conv_pmc_s0.json")
        ks = json.load(open(pm))["kernels"]
        cands = [v for kn, v in ks.items() if kn.startswith("conv7_kernel<bf16_t, 64>") and "hbm_bytes" in v]
        k = cands[0]
        out["traffic"] = round(k["hbm_bytes"])
        out["traffic_source"] = os.path.relpath(pm, ROOT)
    except Exception:
        pass
    return out


def gemm_roofline(device, rows: int = 20000, c: int = 256):
    """The dense GEMMs of a deep-stage Block (ptv3m1:173-248 at 256 channels; N = the ~20000 voxels stage 3 holds at the bench shape): forward
    qkv (c -> 3c), fc1 with its GELU epilogue (c -> 4c), fc2 (4c -> c) on gemm3.h and the weight gradient of fc1 on wgrad3.h.  MFMA-bound by
    SURVEY 8(d): useful flops = 2 N c_in c_out; achieved = flops / launch time (HIP events on the launch stream)."""
    from pointcept_amd import ops

    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(rows, c, generator=g).to(torch.bfloat16).to(device)
    h = torch.randn(rows, 4 * c, generator=g).to(torch.bfloat16).to(device)
    out = {"bound": "mfma", "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "rows": rows, "kernels": {}}

    def line(name, fn, cin, cout):
        ms = _time_launches(fn, iters=20, warm=5)
        fl = 2.0 * rows * cin * cout
        out["kernels"][name] = {"launch_ms": round(ms, 4), "achieved": round(fl / (ms * 1e-3) / 1e12, 1),
                                "frac": round(fl / (ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4), "algorithmic_flops_per_launch": fl}

    w_qkv = (torch.randn(3 * c, 1, c, generator=g) * 0.05).to(torch.bfloat16).to(device)
    b_qkv = torch.zeros(3 * c, device=device)
    line("gemm3 qkv %d->%d" % (c, 3 * c), lambda: ops.spconv_fwd(x, w_qkv, b_qkv, None), c, 3 * c)
    w1 = (torch.randn(4 * c, c, generator=g) * 0.05).to(torch.bfloat16).to(device)
    b1 = torch.zeros(4 * c, device=device)
    line("gemm3 fc1+GELU %d->%d" % (c, 4 * c), lambda: ops.linear_gelu_fwd(x, w1, b1), c, 4 * c)
    w2 = (torch.randn(c, 1, 4 * c, generator=g) * 0.03).to(torch.bfloat16).to(device)
    b2 = torch.zeros(c, device=device)
    line("gemm3 fc2 %d->%d" % (4 * c, c), lambda: ops.spconv_fwd(h, w2, b2, None), 4 * c, c)
    line("wgrad3 fc1 %d->%d (+ the reduction of its partials)" % (c, 4 * c), lambda: ops.spconv_wgrad(x, h, None, want_bias=True), c, 4 * c)
    k = out["kernels"]["gemm3 qkv %d->%d" % (c, 3 * c)]
    out.update(kernel="gemm3_kernel (qkv of a 256-channel Block)", achieved=k["achieved"], frac=k["frac"], launch_ms=k["launch_ms"], traffic=None)
    return out


# ----------------------------------------------------------------------------------------------------------------
# CPU baseline
# ----------------------------------------------------------------------------------------------------------------
def cpu_baseline(sample_points: int, scene_points: int, iters: int, lovasz: bool):
    """The oracle port of the reference model (fp32, flash-branch semantics in fp32 math) on the host
    cores: 1 warm-up + `iters` timed forward+backward of the SAME PT-v3m1 base architecture + criteria on one scene
    of `sample_points` voxels, scaled by voxels to scenes of `scene_points` (attention works on fixed 1024-patches
    and every other op is per-voxel, so the cost is linear in voxels).  kind = "port": the reference's own model file
    needs /root/reference and its un-vendored dependencies, neither exists on the GPU box."""
    from oracle import ptv3_model as om
    from pointcept_amd import synthetic

    cores = min(os.cpu_count() or 1, 64)
    torch.set_num_threads(cores)
    torch.manual_seed(0)
    kw = {k: v for k, v in PTV3_BASE.items() if k not in ("enable_flash", "upcast_attention", "upcast_softmax")}
    net = om.SegmentorV2(20, 64, om.PointTransformerV3(**kw), criteria=("ce", "lovasz") if lovasz else ("ce",))
    net.train()
    batch = {k: torch.from_numpy(v) for k, v in synthetic.collate([synthetic.indoor_scene(0, sample_points)]).items()}
    net(batch)["loss"].backward()  # warm-up (thread pools, allocator)
    times = []
    for _ in range(max(1, iters)):
        net.zero_grad(set_to_none=True)
        t0 = time.perf_counter()
        net(batch)["loss"].backward()
        times.append(time.perf_counter() - t0)
    dt = sum(times) / len(times)
    n = int(batch["offset"][-1])
    value = (n / scene_points) / dt
    return {"value": round(value, 5), "unit": "scenes/s", "cores": cores, "kind": "port",
            "sample": f"1 scene x {n} voxels, 1 warm-up + {len(times)} timed fwd+bwd of PT-v3m1 base fp32 on the CPU oracle "
                      f"(mean {dt:.2f} s, min {min(times):.2f} s), scaled by voxels to {scene_points}-voxel scenes; "
                      "port of the reference model file (the file itself cannot travel to the GPU box)"}


# ----------------------------------------------------------------------------------------------------------------
# the timed loop (shared by both models and the stub)
# ----------------------------------------------------------------------------------------------------------------
def timed_steps(step, steps, warmup, device):
    from pointcept_amd import dp

    loss = None
    for _ in range(warmup):
        loss = step()
    dp.barrier(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    dp.barrier(device)
    dt = time.perf_counter() - t0
    return dp.max_over_ranks(dt, device), loss


def make_step(step_model, opt, batch, amp: str, loss_of, device):
    """One optimizer step as engines/train.py:185-246 runs it: zero_grad, autocast forward, (scaled) backward,
    (unscale + inf check +) optimizer step.  fp16: GradScaler; bf16: no scaler (same exponent range as fp32)."""
    dtype = torch.float16 if amp == "fp16" else torch.bfloat16
    scaler = torch.amp.GradScaler(device.type) if amp == "fp16" else None

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast(device.type, dtype=dtype):
            loss = loss_of(step_model(dict(batch)))
        if scaler is not None:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        return loss

    return step


DUMP_ROWS = 1 << 16       # logit rows kept by --dump-outputs
DUMP_ELEMS = 1 << 20      # gradient / parameter elements kept by --dump-outputs
DUMP_MAX_BYTES = 64 << 20


def _seeded_subset(n: int, k: int, seed: int) -> torch.Tensor:
    """k of range(n) in ascending order, the same for every run and build (all of them when n <= k)"""
    if n <= k:
        return torch.arange(n)
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].sort().values


def dump_outputs(out_dir: str, loss, logits, model) -> dict:
    """What the last timed step handed its caller, as float32 / float64 .npy files (a fixed sample where the full array is large):
      loss.npy          ()                      the step's loss (float64)
      logits.npy        (rows, classes)         the seg head's output, a seeded sample of DUMP_ROWS rows (float32)
      grad_norm.npy     (n_params,)             L2 norm of every parameter's gradient, model.parameters() order (float64)
      grad_sample.npy   (DUMP_ELEMS,)           a seeded sample of all gradients, flattened and concatenated in that order (float32)
      param_sample.npy  (DUMP_ELEMS,)           the same elements of the parameters after the optimizer step (float32)
    Returns {name: shape}."""
    import numpy as np

    params = list(model.parameters())
    grads = [torch.zeros_like(p) if p.grad is None else p.grad for p in params]
    flat_g = torch.cat([g.detach().reshape(-1).float() for g in grads])
    flat_p = torch.cat([p.detach().reshape(-1).float() for p in params])
    pick = _seeded_subset(flat_p.numel(), DUMP_ELEMS, 1).to(flat_p.device)
    logits = logits.detach().reshape(logits.shape[0], -1)
    rows = _seeded_subset(logits.shape[0], DUMP_ROWS, 2).to(logits.device)
    arrays = {
        "loss": np.asarray(float(loss.detach()), dtype=np.float64),
        "logits": logits[rows].float().cpu().numpy(),
        "grad_norm": torch.stack([g.detach().double().norm() for g in grads]).cpu().numpy(),
        "grad_sample": flat_g[pick].cpu().numpy(),
        "param_sample": flat_p[pick].cpu().numpy(),
    }
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed {DUMP_MAX_BYTES}")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def fp16_recipe_in_a_child(args):
    """The same PT-v3m1 step under the reference's own mixed-precision recipe -- fp16 autocast + torch.amp.GradScaler
    (configs/_base_/default_runtime.py:19, engines/train.py:203-231) -- measured by a CHILD process running this file with
    `--amp fp16` (the headline line stays bf16 autocast: same operand width, no scaler).  A child, so that nothing it does can take
    the parent's already measured numbers with it; its one JSON line is read from a pipe."""
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--amp", "fp16", "--steps", "5", "--warmup", "2", "--batch", str(args.batch),
               "--points", str(args.points), "--no-secondary", "--no-cpu-baseline", "--no-fp16-recipe"] + (["--ce-only"] if args.ce_only else [])
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
        res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300)
        line = [ln for ln in res.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
        if res.returncode != 0 or not line:
            return {"error": f"child exit code {res.returncode}"}
        j = json.loads(line[-1])
        return {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "steps": j["steps"], "warmup": j["warmup"],
                "amp": j["config"]["amp"], "final_loss": j["config"]["final_loss"], "measured_by": "child process: bench.py --amp fp16"}
    except Exception as e:
        return {"error": repr(e)}


def build_ptv3_outdoor(args, device, rank):
    """BASELINE configs[4] on one GPU: PT-v3m1 base with in_channels = 4 (coord | strength), 16 classes
    (configs/nuscenes/semseg-pt-v3m1-0-base.py:16,122), LiDAR-like sweeps voxelised at 0.05 m (depth-12 grid), ~200k voxels per scene."""
    from pointcept_amd import synthetic
    from pointcept_amd.point_transformer_v3 import PointTransformerV3
    from pointcept_amd.segmentor import DefaultSegmentorV2

    model = DefaultSegmentorV2(16, 64, PointTransformerV3(**dict(PTV3_BASE, in_channels=4)), criteria=("ce", "lovasz")).to(device).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.05, fused=True)
    batch = synthetic.to_torch(synthetic.collate([synthetic.outdoor_scene(5000 + 1000 * rank + i, azimuth_steps=3300) for i in range(args.batch)]), device)
    return model, opt, batch, (lambda out: out["loss"])


def build_ptv3m2_sonata(args, device, rank):
    """PT-v3m2 with the channel plan of the reference's Sonata configs (configs/sonata/*:45: enc (48, 96, 192, 384, 512), heads (3, 6, 12, 24,
    32), patch 1024, 4 orders) plus a decoder of the same widths and a 20-class head, on the bench batch: the LayerNorm widths 48 / 96 / 192
    / 384 and the 192- / 384- / 768- / 1536-wide MLPs that PT-v3m1 does not have."""
    from pointcept_amd import synthetic
    from pointcept_amd.point_transformer_v3m2 import PointTransformerV3 as PTv3m2
    from pointcept_amd.segmentor import DefaultSegmentorV2

    cfg = dict(in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2), enc_depths=(2, 2, 2, 6, 2),
               enc_channels=(48, 96, 192, 384, 512), enc_num_head=(3, 6, 12, 24, 32), enc_patch_size=(1024,) * 5, dec_depths=(2, 2, 2, 2),
               dec_channels=(48, 96, 192, 384), dec_num_head=(3, 6, 12, 24), dec_patch_size=(1024,) * 4, mlp_ratio=4, qkv_bias=True,
               drop_path=0.3, shuffle_orders=True)
    model = DefaultSegmentorV2(20, 48, PTv3m2(**cfg), criteria=("ce", "lovasz")).to(device).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.05, fused=True)
    batch = synthetic.to_torch(synthetic.indoor_batch(args.batch, args.points, rank=rank), device)
    batch["grid_size"] = 0.02
    return model, opt, batch, (lambda out: out["loss"])


def build_ptv3(args, device, rank):
    from pointcept_amd import synthetic
    from pointcept_amd.point_transformer_v3 import PointTransformerV3
    from pointcept_amd.segmentor import DefaultSegmentorV2

    criteria = ("ce",) if args.ce_only else ("ce", "lovasz")
    model = DefaultSegmentorV2(20, 64, PointTransformerV3(**PTV3_BASE), criteria=criteria).to(device).train()
    # AdamW of scannet/semseg-pt-v3m1-0-base.py:56; fused=True = the same update in one multi-tensor kernel per group
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.05, fused=True)
    batch = synthetic.to_torch(synthetic.indoor_batch(args.batch, args.points, rank=rank), device)
    return model, opt, batch, (lambda out: out["loss"])


def build_spunet(args, device, rank, points):
    from pointcept_amd import functional as PF
    from pointcept_amd import synthetic
    from pointcept_amd.sparse_unet import SpUNetBase

    model = SpUNetBase(6, 20, **SPUNET_BASE).to(device).train()
    # SGD of scannet/semseg-spunet-v1m1-0-base.py:36
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    batch = synthetic.to_torch(synthetic.indoor_batch(args.batch, points, rank=rank), device)
    seg = batch["segment"]
    return model, opt, batch, (lambda logits: PF.cross_entropy(logits, seg, -1))


def build_stub(args, device, rank):
    """CPU stand-in for the launcher test: the DP plumbing is the subject, not the model."""
    from pointcept_amd import dp

    model = torch.nn.Sequential(torch.nn.Linear(6, 32), torch.nn.BatchNorm1d(32), torch.nn.GELU(), torch.nn.Linear(32, 20)).to(device)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    g = torch.Generator().manual_seed(dp.scene_seeds(rank, 1)[0])
    n = 256 * args.batch
    batch = {"feat": torch.randn(n, 6, generator=g), "segment": torch.randint(0, 20, (n,), generator=g)}

    class Wrap(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, d):
            return self.m(d["feat"])

    seg = batch["segment"]
    return Wrap(model), opt, batch, (lambda logits: torch.nn.functional.cross_entropy(logits.float(), seg))


def use_prebuilt_library_if_read_only():
    """The package loads libptcore.so through build(), and builds made before build() skipped its lock when nothing is stale
    open a lock file in the build directory on that first use.  A built tree that belongs to another user (a second build
    compared with this one through --dump-outputs) cannot be written here, so where this user could not take that lock the
    benchmark runs the library that build() made as it is, the path build() takes on a box without hipcc (HIPCC="" names no
    compiler; the ranks and the child process inherit it)."""
    variant = os.environ.get("PTC_LIB_VARIANT", "")
    pkg = os.path.join(ROOT, "pointcept_amd")
    build_dir = os.path.join(pkg, "csrc", "build" + ("_" + variant if variant else ""))
    lock = os.path.join(build_dir, ".lock")
    target = lock if os.path.exists(lock) else build_dir if os.path.isdir(build_dir) else pkg
    if os.path.exists(os.path.join(pkg, f"libptcore_{variant}.so" if variant else "libptcore.so")) and not os.access(target, os.W_OK):
        os.environ["HIPCC"] = ""


def main():
    args = parse()
    use_prebuilt_library_if_read_only()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    from pointcept_amd import dp

    # The ONE JSON line must be the last thing on stdout.  RCCL printf()s a version banner into the C stdout buffer when its first
    # communicator comes up, and that buffer is flushed at process exit -- AFTER the line (seen on the GPU box: profiles/
    # r02_y_ddp_single_rank.txt).  So file descriptor 1 is pointed at stderr for the whole run and the line is written to the
    # saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    rank, local_rank, world = dp.env_rank()
    # one Python process per GPU shares the host: NUMA-local cores and a bounded thread pool per rank (no-op at world size 1)
    affinity = dp.pin_rank_to_cores(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a different GPU count than asked")
    if args.stub:
        device = torch.device("cpu")
        dp.init_distributed(backend="gloo")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
        if torch.cuda.device_count() <= local_rank:
            raise SystemExit(f"bench.py: LOCAL_RANK {local_rank} but only {torch.cuda.device_count()} GPU(s) visible")
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
        dp.init_distributed(backend="nccl", device=device)
    ranks = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    if ranks != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but the process group has {ranks} rank(s)")

    torch.manual_seed(1234)  # identical initial weights on every rank
    points = args.points
    if args.stub:
        model, opt, batch, loss_of = build_stub(args, device, rank)
        metric, workload, amp = "stub steps (launcher / DP plumbing check, not a benchmark)", "stub", "bf16"
    elif args.model == "spunet":
        points = 100000 if args.points == 102400 else args.points
        model, opt, batch, loss_of = build_spunet(args, device, rank, points)
        metric = "scenes/sec (fwd+bwd+optimizer) SpUNet-v1m1 ScanNet-semseg @ 100k voxels"
        workload = f"SpUNet-v1m1 (39.2M params) + CE, fwd+bwd+SGD, {args.batch} scenes x {points} voxels per GPU"
        amp = args.amp
    elif args.model == "ptv3-outdoor":
        model, opt, batch, loss_of = build_ptv3_outdoor(args, device, rank)
        points = int(batch["offset"][-1]) // args.batch
        metric = "scenes/sec (fwd+bwd+optimizer) PT-v3m1 outdoor LiDAR semseg @ ~200k voxels (BASELINE configs[4])"
        workload = f"PT-v3m1 base, in_channels 4, 16 classes, CE + Lovasz, fwd+bwd+AdamW, {args.batch} scenes x ~{points} voxels per GPU"
        amp = args.amp
    elif args.model == "ptv3m2-sonata":
        model, opt, batch, loss_of = build_ptv3m2_sonata(args, device, rank)
        metric = "scenes/sec (fwd+bwd+optimizer) PT-v3m2 (Sonata widths 48..512) semseg @ ~100k pts"
        workload = f"PT-v3m2 enc (48, 96, 192, 384, 512) / dec (48, 96, 192, 384), CE + Lovasz, fwd+bwd+AdamW, {args.batch} scenes x {points} voxels per GPU"
        amp = args.amp
    else:
        model, opt, batch, loss_of = build_ptv3(args, device, rank)
        metric = "scenes/sec (fwd+bwd+optimizer) PTv3 ScanNet-semseg @ ~100k pts"
        workload = ("PT-v3m1 base (46.2M params) + seg head + " + ("CE" if args.ce_only else "CE + Lovasz") + ", fwd+bwd+AdamW, "
                    f"{args.batch} scenes x {points} voxels per GPU, patch 1024, 4 orders")
        amp = args.amp
    n_params = sum(p.numel() for p in model.parameters())
    step_model = dp.wrap_ddp(model, device)   # identity at world 1
    torch.manual_seed(100 + rank)  # order shuffles / DropPath differ per rank, as in training
    step = make_step(step_model, opt, batch, amp, loss_of, device)
    if args.dump_outputs:
        # the logits of the last step: the seg head's output (DefaultSegmentorV2), the model's own output otherwise (SpUNet, stub)
        seen = {}
        hook = getattr(model, "seg_head", model).register_forward_hook(lambda mod, inp, o: seen.__setitem__("logits", o))
    dt, loss = timed_steps(step, args.steps, args.warmup, device)
    last_loss = float(loss.detach())
    dumped = None
    if args.dump_outputs:
        hook.remove()
        if rank == 0:
            dumped = dump_outputs(args.dump_outputs, loss, seen.pop("logits"), model)
    # multi-GPU diagnostics (--full, outside the timed region): every rank's own step time, and the same K steps WITHOUT the gradient
    # exchange (DDP.no_sync) -- the difference is the all-reduce time the overlap with backward did not hide
    per_rank_ms, ms_no_sync = None, None
    if args.full and world > 1 and torch.distributed.is_initialized():
        t = torch.tensor([dt / args.steps * 1e3], dtype=torch.float64, device=device)
        allt = [torch.zeros_like(t) for _ in range(world)]
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        t[0] = (time.perf_counter() - t0) / args.steps * 1e3          # this rank's own clock, no barrier inside
        torch.distributed.all_gather(allt, t)
        per_rank_ms = [round(float(x.item()), 3) for x in allt]
        if hasattr(step_model, "no_sync"):
            with step_model.no_sync():
                dt_ns, _ = timed_steps(step, max(2, args.steps // 2), 1, device)
            ms_no_sync = round(dt_ns / max(2, args.steps // 2) * 1e3, 3)

    if rank == 0:
        out = {
            "metric": metric,
            "value": round(args.batch * world * args.steps / dt, 4),
            "unit": "scenes/s",
            "n_gpus": world,
            "ddp": type(step_model).__name__ == "DistributedDataParallel",
            "rccl_ranks": ranks,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": amp,
            "data": "synthetic",
            "config": {"workload": workload, "global_batch": args.batch * world, "parallelism": f"dp{world}", "params": n_params,
                       "amp": ("fp16 autocast + GradScaler" if amp == "fp16" else "bf16 autocast"), "final_loss": round(last_loss, 4)},
        }
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        if world > 1:
            out["cpu_affinity_rank0"] = affinity
        if per_rank_ms is not None:
            out["per_rank_ms_per_step"] = per_rank_ms
            out["ms_per_step_without_gradient_exchange"] = ms_no_sync
            out["exposed_allreduce_ms_per_step"] = None if ms_no_sync is None else round(out["ms_per_step"] - ms_no_sync, 3)
        if not args.stub and args.model == "ptv3":
            out["config"]["points_per_gpu"] = int(batch["offset"][-1])
            out["config"]["loss"] = "CrossEntropy(ignore_index=-1)" + ("" if args.ce_only else " + LovaszSoftmax")
        # everything below is --full: diagnostics measured after the headline, each in its own try so that none can take the line with it
        if args.full and not args.stub and args.model == "ptv3":
            if args.batch == 8 and args.points == 102400:      # the table was measured on the default workload
                st = step_traffic()
                if st:
                    out["step_traffic_gb"] = st["step_traffic_gb"]
                    out["step_traffic"] = st
            try:
                out["roofline"] = attention_roofline(device, args.batch, args.points)
            except Exception as e:  # never lose the headline number to a diagnostics failure
                out["roofline"] = {"error": repr(e)}
            if not args.no_secondary:
                try:
                    out["roofline_gather"] = gather_roofline(device, batch)
                except Exception as e:
                    out["roofline_gather"] = {"error": repr(e)}
                try:
                    out["roofline_gemm"] = gemm_roofline(device)
                except Exception as e:
                    out["roofline_gemm"] = {"error": repr(e)}
        if args.full and not args.stub and args.model == "ptv3" and world == 1 and not args.no_secondary:
            try:
                del step, step_model, model, opt, batch
                torch.cuda.empty_cache()
                torch.manual_seed(1234)
                m2, o2, b2, l2 = build_spunet(args, device, rank, 100000)
                st2 = make_step(m2, o2, b2, amp, l2, device)
                k2 = max(3, min(args.steps, 10))
                dt2, loss2 = timed_steps(st2, k2, 2, device)
                out["secondary"] = {"metric": "scenes/sec (fwd+bwd+optimizer) SpUNet-v1m1 ScanNet-semseg @ 100k voxels (BASELINE configs[1])",
                                    "value": round(args.batch * k2 / dt2, 4), "unit": "scenes/s", "ms_per_step": round(dt2 / k2 * 1e3, 3),
                                    "steps": k2, "warmup": 2, "final_loss": round(float(loss2.detach()), 4), "amp": f"{amp} autocast",
                                    "workload": f"SpUNet-v1m1 (39.2M params) + CE, fwd+bwd+SGD, {args.batch} scenes x 100000 voxels"}
                if amp == "bf16":
                    # the AMP dtype SURVEY 8(d) names for configs[1] (fp16 autocast + GradScaler, configs/_base_/default_runtime.py:19): the
                    # same model, weights and batch, a fresh optimizer state; the shadows of both dtypes live side by side (functional._CastCache)
                    try:
                        o2h = torch.optim.SGD(m2.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
                        st2h = make_step(m2, o2h, b2, "fp16", l2, device)
                        dt2h, loss2h = timed_steps(st2h, k2, 3, device)
                        out["secondary"]["recipe_fp16"] = {"value": round(args.batch * k2 / dt2h, 4), "unit": "scenes/s", "ms_per_step": round(dt2h / k2 * 1e3, 3),
                                                           "steps": k2, "warmup": 3, "amp": "fp16 autocast + GradScaler",
                                                           "final_loss": round(float(loss2h.detach()), 4)}
                        del st2h, o2h
                    except Exception as e:
                        out["secondary"]["recipe_fp16"] = {"error": repr(e)}
                del st2, m2, o2, b2
            except Exception as e:
                out["secondary"] = {"error": repr(e)}
        if args.full and not args.stub and args.model == "ptv3" and world == 1 and not args.no_secondary:
            try:      # BASELINE configs[4] (outdoor LiDAR, ~200k voxels per scene, depth-12 grid) on this one GPU
                torch.cuda.empty_cache()
                torch.manual_seed(1234)
                m3, o3, b3, l3 = build_ptv3_outdoor(args, device, rank)
                st3 = make_step(m3, o3, b3, amp, l3, device)
                k3 = max(3, min(args.steps, 6))
                dt3, loss3 = timed_steps(st3, k3, 2, device)
                n3 = int(b3["offset"][-1])
                out["secondary_outdoor"] = {"metric": "scenes/sec (fwd+bwd+optimizer) PT-v3m1 outdoor LiDAR semseg @ ~200k voxels (BASELINE configs[4], one GPU)",
                                            "value": round(args.batch * k3 / dt3, 4), "unit": "scenes/s", "ms_per_step": round(dt3 / k3 * 1e3, 3),
                                            "steps": k3, "warmup": 2, "final_loss": round(float(loss3.detach()), 4), "voxels_per_gpu": n3,
                                            "grid_depth": int(b3["grid_coord"].max()).bit_length(),
                                            "workload": f"PT-v3m1 base, in_channels 4, 16 classes, CE + Lovasz, fwd+bwd+AdamW, {args.batch} scenes x ~{n3 // args.batch} voxels"}
                del st3, m3, o3, b3
                torch.cuda.empty_cache()
            except Exception as e:
                out["secondary_outdoor"] = {"error": repr(e)}
        if args.full and not args.stub and args.model == "ptv3" and world == 1 and not args.no_secondary:
            try:      # SURVEY 8(f).2 at the widths the reference ships: PT-v3m2 with configs/sonata's channel plan on the bench batch
                torch.cuda.empty_cache()
                torch.manual_seed(1234)
                m4, o4, b4, l4 = build_ptv3m2_sonata(args, device, rank)
                st4 = make_step(m4, o4, b4, amp, l4, device)
                k4 = max(3, min(args.steps, 6))
                dt4, loss4 = timed_steps(st4, k4, 2, device)
                out["secondary_f2"] = {"metric": "scenes/sec (fwd+bwd+optimizer) PT-v3m2 (Sonata widths 48..512) semseg @ ~100k pts, one GPU",
                                       "value": round(args.batch * k4 / dt4, 4), "unit": "scenes/s", "ms_per_step": round(dt4 / k4 * 1e3, 3),
                                       "steps": k4, "warmup": 2, "final_loss": round(float(loss4.detach()), 4),
                                       "workload": f"PT-v3m2 enc (48, 96, 192, 384, 512) / dec (48, 96, 192, 384), head_dim 16, CE + Lovasz, fwd+bwd+AdamW, "
                                                   f"{args.batch} scenes x {args.points} voxels; LayerNorm / GEMM widths outside PT-v3m1's on the engine's generic kernels"}
                del st4, m4, o4, b4
                torch.cuda.empty_cache()
            except Exception as e:
                out["secondary_f2"] = {"error": repr(e)}
        if args.full and not args.stub and args.model == "ptv3" and world == 1 and amp == "bf16" and not args.no_secondary and not args.no_fp16_recipe:
            out["recipe_fp16"] = fp16_recipe_in_a_child(args)
        if args.full and not args.stub and args.model == "ptv3" and world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args.cpu_sample_points, args.points, args.cpu_iters, not args.ce_only)
            except Exception as e:
                out["cpu_baseline"] = {"error": repr(e)}
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if torch.distributed.is_initialized():
        dp.barrier(device)
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
