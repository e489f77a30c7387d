#!/usr/bin/env python
"""One OA-CNNs training step (configs/scannet/semseg-oacnns-v1m1-0-base.py backbone + cross entropy, fwd + bwd + AdamW) on a
synthetic ScanNet batch, A/B of the adaptive aggregation: csrc/cluster_agg.hip against the reference's ATen expression
(PTC_OACNN_AGG=0).  Each leg runs in a child process (the switch is read at import).  Prints one JSON line per leg.

    python tools/oacnns_step.py [--scenes 4] [--points 100000] [--steps 5] [--warmup 2] [--amp bf16|fp16|none]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(args):
    import torch

    from pointcept_amd import config
    from pointcept_amd import functional as PF
    from pointcept_amd import synthetic
    from pointcept_amd.oacnns import OACNNs

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_oacnns import SCANNET

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = OACNNs(**SCANNET).to(dev).train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.02)
    b = synthetic.to_torch(synthetic.collate([synthetic.indoor_scene(51 + i, args.points) for i in range(args.scenes)]), dev)
    b["feat"] = torch.cat([b["feat"], b["feat"][:, :3]], 1).contiguous()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "none": None}[args.amp]
    scaler = torch.amp.GradScaler("cuda") if dt == torch.float16 else None

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dt or torch.float32, enabled=dt is not None):
            loss = PF.cross_entropy(net(dict(b)).float(), b["segment"], -1)
        if scaler:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        return loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"agg": "kernel" if config.OACNN_AGG else "torch (PTC_OACNN_AGG=0)", "amp": args.amp, "scenes": args.scenes,
                      "voxels": int(b["feat"].shape[0]), "ms_per_step": round(e0.elapsed_time(e1) / args.steps, 2),
                      "loss": round(float(loss.detach()), 5), "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--amp", default="bf16", choices=["bf16", "fp16", "none"])
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    for flag in ("1", "0"):
        env = dict(os.environ, PTC_OACNN_AGG=flag)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg"] + sys.argv[1:], env=env, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"leg PTC_OACNN_AGG={flag} failed with {r.returncode}")


if __name__ == "__main__":
    main()
