#!/usr/bin/env python
"""PointGroup on the ScanNet v1m1 config (configs/scannet/insseg-pointgroup-v1m1-0-spunet-base.py: SpUNet-v1m1, 96 channels, radius
1.5 voxels, 50 / 100 points) at 2 x 100 000 synthetic points: csrc/pg_cluster.hip against PTC_PG_CLUSTER=0 (the chunked brute-force
torch ball query, the host BFS and the reference's loss expression).  Prints one JSON line per measurement:

* ops: ball query and clustering alone, realistic centres (offsets predicted to 5 cm) and collapsed centres (exact offsets: every
  instance on one point, every list truncated);
* eval: one eval forward of the model with those centres (heads pinned, so both legs cluster the same predictions);
* train: one bf16 training step (fwd + bwd + SGD), both legs from the same weights.
Times: median, min and max over the timed runs (torch legs: `--torch-steps` runs after one warm-up).
The host BFS of the collapsed case is a Python loop over ~10^8 list entries at full size: that leg runs at `--collapsed-torch-points`.

    python tools/pointgroup_step.py [--points 100000] [--steps 5] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPUNET = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2))
PG_CFG = dict(backbone=SPUNET, backbone_out_channels=96, semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=(-1, 0, 1),
              instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300, cluster_propose_points=100, cluster_min_points=50)


def timed(fn, steps, warmup):
    """wall-clock ms of fn() + a device synchronize: (median, min, max) over `steps` runs after `warmup` runs"""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return dict(ms=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3), runs=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--collapsed-torch-points", type=int, default=10000)
    args = ap.parse_args()
    import torch

    from pointcept_amd import config
    from pointcept_amd import functional as PF
    from pointcept_amd import ops
    from pointcept_amd import synthetic
    from pointcept_amd.point_group import PointGroup
    from pointcept_amd.structure import offset2batch

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = PointGroup(**PG_CFG).to(dev)
    batch = synthetic.to_torch(synthetic.indoor_instance_batch((61, 62), (args.points, args.points)), dev)
    n = batch["coord"].shape[0]
    gt = batch["instance_centroid"] - batch["coord"]
    gt = torch.where(batch["instance"][:, None] >= 0, gt, torch.zeros_like(gt))
    logits = torch.nn.functional.one_hot(batch["segment"].clamp(min=0), 20).float() * 4
    logits = logits + torch.randn(n, 20, device=dev) * 0.5
    realistic = gt + torch.randn_like(gt) * 0.05          # offsets predicted to 5 cm
    ign = torch.isin(logits.argmax(1), torch.tensor([0, 1], device=dev))
    batch_idx = torch.where(ign, -1, offset2batch(batch["offset"], n))
    label = torch.where(ign, -1, logits.argmax(1)).int()
    sizes = (n, int(batch["offset"][0]))

    def ops_leg(kind, bias, kernel, limit=None):
        centres = ((batch["coord"] + bias) / 0.02)
        b, lab = batch_idx, label
        if limit is not None:              # the first `limit` points of each scene
            keep = torch.cat([torch.arange(limit, device=dev), sizes[1] + torch.arange(limit, device=dev)])
            centres, b, lab = centres[keep], b[keep], lab[keep]
        keep_pts = torch.nonzero(b >= 0)[:, 0]
        c_, b_, l_ = centres[keep_pts].contiguous(), b[keep_pts].int().contiguous(), lab[keep_pts].contiguous()
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(b_, minlength=2), 0)]).cpu()

        def run():
            if kernel:
                idx, sl, _ = ops.pg_ball_query(c_, b_, 2, 1.5)
                return ops.pg_cluster(l_, idx, sl, 50)
            idx, sl = PF.pg_ball_query_torch(c_, b_, off, 1.5)
            return PF.pg_bfs_cluster_host(l_.cpu(), idx.cpu(), sl.cpu(), 50)

        t = timed(run, args.steps if kernel else args.torch_steps, args.warmup if kernel else 1)
        ci, co = run()
        stages = {}
        if kernel:                         # the two halves on their own
            stages["ball_query"] = timed(lambda: ops.pg_ball_query(c_, b_, 2, 1.5), args.steps, args.warmup)
            idx, sl, n_trunc = ops.pg_ball_query(c_, b_, 2, 1.5)
            stages["cluster"] = timed(lambda: ops.pg_cluster(l_, idx, sl, 50), args.steps, args.warmup)
            stages["truncated_lists"] = n_trunc
            stages["list_entries"] = int(idx.numel())
        print(json.dumps({"what": f"ops ball query + cluster, {kind}", "path": "kernel" if kernel else "torch (PTC_PG_CLUSTER=0)",
                          "points": int(c_.shape[0]), **t, "clusters": int(co.numel() - 1), **stages}), flush=True)

    for kernel in (True, False):
        ops_leg("realistic", realistic, kernel)
    ops_leg("collapsed", gt, True)
    ops_leg("collapsed", gt, True, limit=args.collapsed_torch_points)
    ops_leg("collapsed", gt, False, limit=args.collapsed_torch_points)

    def eval_leg(kind, bias, kernel):
        config.PG_CLUSTER = kernel
        net.eval()
        net.heads = lambda f: (bias, logits)
        with torch.no_grad():
            def run():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return net(dict(batch))

            t = timed(run, args.steps if kernel else args.torch_steps, args.warmup if kernel else 1)
            out = run()
        del net.heads
        print(json.dumps({"what": f"eval forward, {kind} centres", "path": "kernel" if kernel else "torch (PTC_PG_CLUSTER=0)",
                          "points": n, **t, "proposals": int(out["pred_masks"].shape[0])}), flush=True)

    for kernel in (True, False):
        eval_leg("realistic", realistic, kernel)
    eval_leg("collapsed", gt, True)

    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    for kernel in (True, False):         # both legs from the same weights and a fresh optimizer
        config.PG_CLUSTER = kernel
        net.load_state_dict(sd0)
        net.train()
        opt = torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
        last = {}

        def step():
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = net(dict(batch))
            out["loss"].backward()
            opt.step()
            last["loss"] = out["loss"].detach()

        t = timed(step, 2 * args.steps, args.warmup)
        print(json.dumps({"what": "bf16 train step", "path": "kernel" if kernel else "torch (PTC_PG_CLUSTER=0)", "points": n, **t,
                          "loss": round(float(last["loss"]), 5), "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 2)}),
              flush=True)
    config.PG_CLUSTER = True


if __name__ == "__main__":
    main()
