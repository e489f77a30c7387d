"""The device-side augmentations (csrc/augment.hip, pointcept_amd/augment.py) at one synthetic indoor scene of ~200 000 points: the
ScanNet training chain of configs/scannet/semseg-pt-v3m1-0-base.py:100-136 (CenterShift ... ChromaticJitter, GridSample, SphereCrop,
CenterShift, NormalizeColor, Collect), every gate open, on three paths:

  engine  augment.Compose on the kernels;
  twin    the same Compose with PTC_AUGMENT=0 (the torch twin, op by op in fp32) on the same GPU in the same process, alternating;
  numpy   the augmentations of the chain (up to GridSample) restated in numpy / scipy on one CPU core, as the reference's dataloader
          workers run them.

Wall time per scene (the call plus a device synchronise: the elastic stages' host reads are part of it), median [min .. max] of the
repeats, GPU kernel launches of one call (torch.profiler), the peak allocation of one call -- and each transform alone on both GPU paths.
`--parity` instead writes the engine's and the twin's errors against the reference golden per case (tests/test_gpu_augment.py).

    python tools/augment_step.py [--points 200000] [--reps 9] [--out profiles/augment_step.txt]
    python tools/augment_step.py --parity --out profiles/augment_parity.txt

Each measurement runs in a child process of its own under a time limit; the parent never touches the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AUGMENT = [
    dict(type="CenterShift", apply_z=True),
    dict(type="RandomDropout", dropout_ratio=0.2, dropout_application_ratio=0.2),
    dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], p=0.5),
    dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="x", p=0.5),
    dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="y", p=0.5),
    dict(type="RandomScale", scale=[0.9, 1.1]),
    dict(type="RandomFlip", p=0.5),
    dict(type="RandomJitter", sigma=0.005, clip=0.02),
    dict(type="ElasticDistortion", distortion_params=[[0.2, 0.4], [0.8, 1.6]]),
    dict(type="ChromaticAutoContrast", p=0.2, blend_factor=None),
    dict(type="ChromaticTranslation", p=0.95, ratio=0.05),
    dict(type="ChromaticJitter", p=0.95, std=0.05),
]
TAIL = [
    dict(type="GridSample", grid_size=0.02, hash_type="fnv", mode="train", return_grid_coord=True),
    dict(type="SphereCrop", point_max=102400, mode="random"),
    dict(type="CenterShift", apply_z=False),
    dict(type="NormalizeColor"),
    dict(type="ToTensor"),
    dict(type="Collect", keys=("coord", "grid_coord", "segment"), feat_keys=("color", "normal")),
]


def draws(n, device, seed=0):
    """every gate open, the scalars fixed, the noise from seeds: engine and twin do the same work in every repeat"""
    import torch

    keep = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:int(n * 0.8)].to(device)
    return [None, dict(gate=0.0, index=keep), dict(gate=0.0, angle=0.37), dict(gate=0.0, angle=0.01), dict(gate=0.0, angle=-0.008),
            dict(scale=1.04), dict(x=0.1, y=0.9), dict(seed=11), dict(gate=0.0, seed=12), dict(gate=0.0, blend=0.6),
            dict(gate=0.0, tr=[0.2, 0.5, 0.9]), dict(gate=0.0, seed=13)]


def numpy_chain(sc, reps):
    """the augmentations of the chain in numpy / scipy, written from the reference's behaviour; -> seconds per repeat"""
    import numpy as np
    import scipy.interpolate
    import scipy.ndimage

    def rot(axis, a):
        c, s = np.cos(a), np.sin(a)
        return np.array({"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis])

    def elastic(coords, g, mag, rng):
        mn = coords.min(0)
        dim = ((coords - mn).max(0) // g).astype(int) + 3
        noise = rng.standard_normal((*dim, 3)).astype(np.float32)
        for _ in range(2):
            for shape in ((3, 1, 1, 1), (1, 3, 1, 1), (1, 1, 3, 1)):
                noise = scipy.ndimage.convolve(noise, np.ones(shape, dtype="float32") / 3, mode="constant", cval=0)
        ax = [np.linspace(a, b, d) for a, b, d in zip(mn - g, mn + g * (dim - 2), dim)]
        return coords + scipy.interpolate.RegularGridInterpolator(ax, noise, bounds_error=False, fill_value=0)(coords) * mag

    times = []
    for r in range(reps):
        rng = np.random.default_rng(r)
        coord, normal, color = sc["coord"].copy(), sc["normal"].copy(), sc["color"].copy()
        t0 = time.perf_counter()
        lo, hi = coord.min(0), coord.max(0)
        coord -= [(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, lo[2]]
        idx = rng.choice(len(coord), int(len(coord) * 0.8), replace=False)
        coord, normal, color = coord[idx], normal[idx], color[idx]
        for axis, a, centre in (("z", 0.37, [0, 0, 0]), ("x", 0.01, None), ("y", -0.008, None)):
            R = rot(axis, a * np.pi)
            c = (coord.min(0) + coord.max(0)) / 2 if centre is None else np.asarray(centre, dtype=float)
            coord = (coord - c) @ R.T + c
            normal = normal @ R.T
        coord = coord * 1.04
        coord[:, 0] = -coord[:, 0]
        normal[:, 0] = -normal[:, 0]
        coord += np.clip(0.005 * rng.standard_normal(coord.shape), -0.02, 0.02)
        for g, mag in ((0.2, 0.4), (0.8, 1.6)):
            coord = elastic(coord, g, mag, rng)
        lo, hi = color.min(0, keepdims=True), color.max(0, keepdims=True)
        scale = 255 / np.where(hi > lo, hi - lo, 255)
        color = 0.4 * color + 0.6 * (color - lo) * scale
        color = np.clip((np.array([[0.2, 0.5, 0.9]]) - 0.5) * 255 * 2 * 0.05 + color, 0, 255)
        color = np.clip(rng.standard_normal(color.shape) * 0.05 * 255 + color, 0, 255)
        times.append(time.perf_counter() - t0)
    return times


def child(what, points, reps):
    import numpy as np
    import torch

    from pointcept_amd import augment, config, synthetic

    if what == "parity":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_gpu_augment as A

        print("RESULT " + json.dumps(dict(table=A.parity_table(torch.device("cuda")))))
        return
    sc = synthetic.indoor_scene(77, point_max=points)
    sc = dict(coord=sc["coord"] + np.float32([1.5, -3.0, 0.4]), normal=np.ascontiguousarray(sc["feat"][:, 3:]),
              color=np.floor(sc["feat"][:, :3] * 255).astype(np.float32), segment=sc["segment"])
    n = sc["coord"].shape[0]
    res = dict(points=n)
    if what == "numpy":
        os.environ["OMP_NUM_THREADS"] = "1"
        torch.set_num_threads(1)
        try:
            res["numpy_s"] = numpy_chain({k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in sc.items()}, max(reps // 3, 2))
        except ImportError as e:
            res["numpy_error"] = str(e)
        print("RESULT " + json.dumps(res))
        return
    dev = torch.device("cuda")
    data = {k: torch.from_numpy(v).to(dev) for k, v in sc.items()}
    dr = draws(n, dev)
    full = augment.Compose(AUGMENT + TAIL)
    full_draws = dr + [None, 1234, None, None, None, None]

    def timed(fn, kernels):
        config.AUGMENT_KERNELS = kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def measure(fn):
        out = dict(ms={True: [], False: []}, peak={}, launches={})
        for kernels in (True, False):
            timed(fn, kernels), timed(fn, kernels)
        for _ in range(reps):                       # alternating, so that drift hits both sides alike
            for kernels in (True, False):
                out["ms"][kernels].append(timed(fn, kernels))
        for kernels in (True, False):
            config.AUGMENT_KERNELS = kernels
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            out["peak"][kernels] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            try:
                from torch.profiler import ProfilerActivity, profile

                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                out["launches"][kernels] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
            except Exception as e:       # no profiler on this build: the engine's own accounting is still reported
                out["launches"][kernels] = f"n/a ({type(e).__name__})"
        return dict(engine_ms=out["ms"][True], twin_ms=out["ms"][False], engine_peak=out["peak"][True], twin_peak=out["peak"][False],
                    engine_launches=out["launches"][True], twin_launches=out["launches"][False])

    if what == "chain":
        res["chain"] = measure(lambda: full(dict(data), full_draws))
        aug = augment.Compose(AUGMENT)
        res["augment"] = measure(lambda: aug(dict(data), dr))
        config.AUGMENT_KERNELS = True
        aug(dict(data), dr)
        res["planned_launches"] = aug.last_launches
    else:                                            # every transform alone
        res["single"] = {}
        for i, (cfg, d) in enumerate(zip(AUGMENT, dr)):
            if cfg["type"] == "RandomDropout":
                continue                             # torch indexing on both paths
            one = augment.Compose([cfg])
            res["single"][f"{i:02d} {cfg['type']}" + (f"({cfg['axis']})" if "axis" in cfg else "")] = measure(lambda: one(dict(data), [d]))
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.points, a.reps)
    fmt = lambda v: f"{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]"      # noqa: E731
    lines = []
    for what in (["parity"] if a.parity else ["chain", "single", "numpy"]):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", what, "--points", str(a.points),
               "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            lines.append(f"{what}: child failed with status {r.returncode}: {r.stderr[-600:]}")
            print(lines[-1])
            if r.returncode in (124, 134, 137, 139, -6, -11):
                break                               # a fault or a hang: nothing more is started on the GPU
            continue
        res = json.loads(got[0][7:])
        if what == "parity":
            lines += ["max abs error against the float64 golden of the reference's own classes (tests/golden/augment.npz), per case and output:",
                      "engine (Compose fused, transforms one by one), the fp32 torch twin, the engine's bound max(2 x twin, 2^-23 max|golden|)",
                      "and the twin's bound 16 x 2^-24 x max|value| per transform", res["table"]]
        elif what == "chain":
            lines.append(f"one synthetic indoor scene of {res['points']} points; wall ms per scene including the device synchronise, median "
                         f"[min .. max] of {a.reps} alternating repeats; launches = GPU kernels of one call; peak = allocation of one call")
            for key, title in (("chain", "whole training list (augmentations, GridSample, SphereCrop, CenterShift, NormalizeColor, Collect)"),
                               ("augment", "the augmentations alone (CenterShift ... ChromaticJitter)")):
                m = res[key]
                k, t = m["engine_ms"], m["twin_ms"]
                verdict = "faster beyond the spread" if max(k) < min(t) else "slower beyond the spread" if min(k) > max(t) else "within the spread"
                lines.append(f"{title}:")
                lines.append(f"  engine        {fmt(k)} ms  launches {m['engine_launches']}  peak {m['engine_peak']:.1f} MB")
                lines.append(f"  PTC_AUGMENT=0 {fmt(t)} ms  launches {m['twin_launches']}  peak {m['twin_peak']:.1f} MB   -> engine {verdict}")
            lines.append(f"  launches of ptc_aug_* kernels planned by Compose for the augmentations: {res['planned_launches']}")
        elif what == "single":
            lines.append("each transform alone (its own launches, one flush):")
            for name, m in res["single"].items():
                k, t = m["engine_ms"], m["twin_ms"]
                verdict = "faster" if max(k) < min(t) else "SLOWER" if min(k) > max(t) else "within the spread"
                lines.append(f"  {name:28s} engine {fmt(k)}  twin {fmt(t)}  launches {m['engine_launches']} | {m['twin_launches']}  -> {verdict}")
        else:
            if "numpy_s" in res:
                lines.append(f"numpy / scipy, one CPU core, the augmentations alone: {fmt([1e3 * v for v in res['numpy_s']])} ms per scene")
            else:
                lines.append(f"numpy / scipy path not measured: {res.get('numpy_error')}")
        print("\n".join(lines[-12:]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
