"""SGIFormer-v1m1 at the ScanNet++ config's decoder shape (configs/scannetpp/insseg-sgiformer-v1m1-0-ptv3-base.py: PT-v3m1 base,
84 + 1 classes, 200 + 200 queries, d_model 256, 8 heads, 3 layers, gelu, attention mask, iter_matcher) on synthetic indoor scenes with
grid-cell superpoints: everything after the backbone (superpoint pooling, decoder, targets, the four Hungarian levels, losses; forward +
backward) and the whole train step, kernel path (csrc/sgiformer.hip) against PTC_SGI=0 (the reference's expression in torch: a loop
over scenes, dense attention probabilities, [Lq, M] BCE maps, the [N, instances] one-hot) in one process, alternating, with the spread
of the repeats and the peak allocation of both.

    python tools/sgiformer_step.py [--scenes 3] [--points 60000] [--cell 0.18] [--reps 5] [--out profiles/sgiformer_step.txt]

Each measurement runs in a child process of its own under a time limit; the parent never touches the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NUM_CLASSES = 84
BACKBONE = dict(type="PT-v3m1", in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2), enc_depths=(2, 2, 2, 6, 2),
                enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32), enc_patch_size=(1024,) * 5, dec_depths=(2, 2, 2, 2),
                dec_channels=(64, 64, 128, 256), dec_num_head=(4, 4, 8, 16), dec_patch_size=(1024,) * 4, drop_path=0.3, enable_flash=True)
DECODER = dict(num_classes=NUM_CLASSES, in_channel=64, dec_num_layer=3, num_sample_query=200, num_learn_query=200, d_model=256, nhead=8,
               hidden_dim=1024, dropout=0.0, activation_fn="gelu", attn_mask=True, use_score=False, alpha=0.4)
CRITERIA = dict(matcher=dict(type="HungarianMatcher", costs=[dict(type="QueryClassificationCost", weight=0.5), dict(type="MaskBCECost", weight=1.0),
                                                             dict(type="MaskDiceCost", weight=1.0)]),
                loss_weight=[0.8, 1.0, 1.0, 0.5, 0.4, 0.4], num_classes=NUM_CLASSES, non_object_weight=0.1, fix_dice_loss_weight=False,
                iter_matcher=True, fix_mean_loss=True)
STAGES = ("decoder", "step")


def child(what, scenes, points, cell, reps, amp):
    import torch

    from pointcept_amd import config, synthetic
    from pointcept_amd.sgiformer import SGIFormer

    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = SGIFormer(backbone=BACKBONE, decoder=DECODER, criteria=CRITERIA, topk_insts=300, semantic_num_classes=NUM_CLASSES).to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    b = synthetic.to_torch(synthetic.indoor_superpoint_batch([300 + i for i in range(scenes)], [points] * scenes, cell), dev)
    cast = torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp)
    with torch.no_grad(), cast:
        feat = model.backbone(dict(b)).feat.float()

    class Fixed(torch.nn.Module):                    # the backbone's features of this batch, as a leaf
        def forward(self, data):
            from pointcept_amd.structure import Point

            p = Point(data)
            p.feat = feat.detach().clone().requires_grad_()
            return p

    backbone = model.backbone
    info = {}

    def decoder_and_criteria():
        model.backbone = Fixed()
        try:
            with cast:
                out = model(dict(b))
            out["loss"].backward()
        finally:
            model.backbone = backbone

    def train_step():
        opt.zero_grad(set_to_none=True)
        with cast:
            out = model(dict(b))
        out["loss"].backward()
        opt.step()

    fn = dict(decoder=decoder_and_criteria, step=train_step)[what]
    with torch.no_grad():
        sp = torch.unique(torch.repeat_interleave(torch.arange(scenes, device=dev), torch.diff(b["offset"], prepend=b["offset"].new_zeros(1))) << 48
                          | b["superpoint"]).numel()
    res = {"points": int(b["offset"][-1]), "superpoints": int(sp), "instances": int(sum(len(torch.unique(i[i >= 0])) for i in torch.tensor_split(
        b["instance"].cpu(), b["offset"][:-1].cpu())))}
    times = {True: [], False: []}
    for kernels in (True, False):                  # warm-up of both sides
        config.SGI_KERNELS = kernels
        fn()
        fn()
    for _ in range(reps):                          # alternating, so that drift hits both sides alike
        for kernels in (True, False):
            config.SGI_KERNELS = kernels
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[kernels].append(e0.elapsed_time(e1))
    res["kernel_ms"], res["torch_ms"] = times[True], times[False]
    for kernels in (True, False):
        config.SGI_KERNELS = kernels
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        res["peak_mb_kernel" if kernels else "peak_mb_torch"] = (torch.cuda.max_memory_allocated() - base) / 2**20
    res.update(info)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=3)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--cell", type=float, default=0.18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fp32", action="store_true", help="no autocast (the shipped config trains under AMP)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.scenes, a.points, a.cell, a.reps, not a.fp32)
    lines = [f"SGIFormer-v1m1, ScanNet++ decoder shape (84 + 1 classes, 200 + 200 queries, d_model 256, 8 heads, 3 layers) on PT-v3m1 base: "
             f"{a.scenes} scenes x {a.points} points before voxelisation, superpoints = {a.cell} m grid cells x instance, "
             f"{'fp32' if a.fp32 else 'bf16 autocast'}; median [min .. max] of {a.reps} alternating repeats, ms, each one event-timed call "
             f"(forward + backward) including its host reads and scipy's assignments; comparison side = PTC_SGI=0 on the same build"]
    for what in STAGES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", what, "--scenes", str(a.scenes),
               "--points", str(a.points), "--cell", str(a.cell), "--reps", str(a.reps)] + (["--fp32"] if a.fp32 else [])
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            lines.append(f"{what}: child failed with status {r.returncode}: {r.stderr[-600:]}")
            print(lines[-1])
            if r.returncode in (124, 134, 137, 139, -6, -11):
                break                                   # a fault or a hang: nothing more is started on the GPU
            continue
        res = json.loads(got[0][7:])
        fmt = lambda v: f"{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]"  # noqa: E731
        kt, tt = res["kernel_ms"], res["torch_ms"]
        verdict = "faster beyond the spread" if max(kt) < min(tt) else "slower beyond the spread" if min(kt) > max(tt) else "within the spread"
        name = "decoder + criteria" if what == "decoder" else "train step"
        lines.append(f"{name:19s} kernels {fmt(kt)}   PTC_SGI=0 {fmt(tt)}   -> {verdict}   ({res['points']} points, {res['superpoints']} "
                     f"superpoints, {res['instances']} instances)")
        print(lines[-1])
        lines.append(f"{'':19s} peak allocation above the resident state: kernels {res['peak_mb_kernel']:.1f} MB, PTC_SGI=0 {res['peak_mb_torch']:.1f} MB")
        print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
