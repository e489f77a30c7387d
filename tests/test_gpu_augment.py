"""-m gpu: the device-side point augmentations (csrc/augment.hip; pointcept_amd/augment.py).  The check_* bodies take a device and
`kernels` (None: the device decides, True: the kernels whatever the device -- tests/test_augment_cpu.py runs them on the host emulation,
False: the torch twin).

Yardstick: tests/golden/augment.npz, the reference's own transform classes run in float64 on the scenes of scene() with every random
value they drew recorded (tests/golden/make_golden_augment.py).  The recorded values are injected as `draw=`, so engine, twin and
reference see the same draws.  Bounds, set before any kernel figure was seen:
  engine  max abs error of an output <= max(2 x the max abs error of the fp32 torch twin on the same case, 2^-23 x max |golden|): the
          engine rounds a double-composed affine once, so it must not be less accurate than rounding after every op; the factor 2
          covers FMA contraction and another order in the 3-term dot products and the 8-term trilinear sum.
  twin    max abs error <= 16 x 2^-24 x max |value| (input and golden) per transform of the chain.
Every figure is printed before it is asserted; parity_table() collects them for profiles/augment_parity.txt (tools/augment_step.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pointcept_amd import augment as AUG  # noqa: E402
from pointcept_amd import config  # noqa: E402
from pointcept_amd import ops  # noqa: E402
from pointcept_amd._lib import PtcoreError  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz")
TILE = 1024            # csrc/augment.hip AU_TILE: points per workgroup
POINT_KEYS = ("coord", "normal", "color")


def dev():
    return torch.device("cuda")


def scene(kind, n, seed):
    """dict of numpy arrays: coord / normal / color fp32 [n, 3], segment int64 [n].
    box: a box of 4 x 3 x 2.5 m away from the origin;  diag: a right triangle whose long side runs along a diagonal (the box of the cloud rotated
    about z is far from the rotated box);  flat: z extent 0;  lattice: coordinates on multiples of 2^-6 with extents exactly (0.5, 0.75, 0.375) and
    points on the upper faces;  const_channel: colours with a constant green channel;  const_color: all colours equal."""
    r = np.random.RandomState(seed * 1009 + n)
    coord = r.uniform(0, 1, (n, 3)) * [4.0, 3.0, 2.5] + [3.0, -2.0, 1.0]
    if kind == "diag":
        a, b = r.uniform(0, 1, n), r.uniform(0, 1, n)
        fold = a + b > 1
        a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
        coord = np.stack([6 * a, 6 * b, r.uniform(0, 0.5, n)], 1) + [1.0, 2.0, 0.5]
    elif kind == "flat":
        coord[:, 2] = 1.5
    elif kind == "lattice":
        coord = np.stack([r.randint(0, 33, n), r.randint(0, 49, n), r.randint(0, 25, n)], 1) / 64.0 + [1.0, -2.0, 0.25]
        if n >= 4:
            coord[0] = [1.0, -2.0, 0.25]
            coord[1] = [1.5, -1.25, 0.625]            # the upper corner: offsets that are exact multiples of g = 0.25 on x and y
            coord[2] = [1.5, -2.0, 0.5]
            coord[3] = [1.25, -1.25, 0.25]
    normal = r.normal(size=(n, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    color = np.floor(r.uniform(0, 256, (n, 3)))
    if kind == "const_channel":
        color[:, 1] = 77.0
    elif kind == "const_color":
        color[:] = [12.0, 200.0, 31.0]
    return dict(coord=coord.astype(np.float32), normal=normal.astype(np.float32), color=color.astype(np.float32),
                segment=r.randint(0, 20, n).astype(np.int64))


def _rot(axis, center, angle=None):
    return dict(type="RandomRotate", angle=[-1, 1] if angle is None else angle, axis=axis, center=center, always_apply=True)


SCANNET_CHAIN = [            # configs/scannet/semseg-pt-v3m1-0-base.py:100-116, up to (not including) GridSample
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
# forced scalar draws (python's random.random / numpy's scalar rand()) so that every gate of the chain opens: dropout, three rotations,
# elastic; flip x only, autocontrast on with blend 0.6, translation and colour jitter on
CHAIN_FORCED = dict(random=[0.1, 0.1, 0.1, 0.1, 0.1], rand=[0.2, 0.7, 0.1, 0.6, 0.3, 0.3])
# one point: the dropout stays closed (the reference would keep int(0.8) = 0 points) and the autocontrast returns before it draws a blend
ONE_POINT_FORCED = dict(random=[0.9, 0.1, 0.1, 0.1, 0.1], rand=[0.2, 0.7, 0.1, 0.3, 0.3])

# name -> (scene kind, n, seed, config list, forced scalar draws, the keys that are compared)
CASES = {
    "center_shift_z": ("box", 129, 1, [dict(type="CenterShift", apply_z=True)], None, ("coord",)),
    "center_shift_xy": ("box", 129, 2, [dict(type="CenterShift", apply_z=False)], None, ("coord",)),
    "center_shift_one_point": ("box", 1, 3, [dict(type="CenterShift", apply_z=True)], None, ("coord",)),
    "random_shift": ("box", 129, 4, [dict(type="RandomShift", shift=((-0.2, 0.2), (-0.2, 0.2), (-0.1, 0.3)))], None, ("coord",)),
    "rotate_x_given": ("box", 129, 5, [_rot("x", [0.5, -1.0, 2.0])], None, ("coord", "normal")),
    "rotate_y_given": ("box", 129, 6, [_rot("y", [0.5, -1.0, 2.0])], None, ("coord", "normal")),
    "rotate_z_given": ("box", 129, 7, [_rot("z", [0, 0, 0])], None, ("coord", "normal")),
    "rotate_x_box": ("box", 129, 8, [_rot("x", None)], None, ("coord", "normal")),
    "rotate_y_box": ("box", 129, 9, [_rot("y", None)], None, ("coord", "normal")),
    "rotate_z_box": ("box", 129, 10, [_rot("z", None)], None, ("coord", "normal")),
    "rotate_then_rotate_box": ("diag", 129, 11, [_rot("z", [0, 0, 0], [0.2, 0.3]), _rot("z", None, [0.4, 0.6])], None, ("coord", "normal")),
    "rotate_target_angle": ("box", 129, 12, [dict(type="RandomRotateTargetAngle", always_apply=True)], None, ("coord", "normal")),
    "flip_x": ("box", 129, 13, [dict(type="RandomFlip", p=0.5)], dict(rand=[0.1, 0.9]), ("coord", "normal")),
    "flip_y": ("box", 129, 14, [dict(type="RandomFlip", p=0.5)], dict(rand=[0.9, 0.1]), ("coord", "normal")),
    "flip_xy": ("box", 129, 15, [dict(type="RandomFlip", p=0.5)], dict(rand=[0.1, 0.1]), ("coord", "normal")),
    "scale": ("box", 129, 16, [dict(type="RandomScale", scale=[0.9, 1.1])], None, ("coord",)),
    "scale_anisotropic": ("box", 129, 17, [dict(type="RandomScale", scale=[0.5, 2.0], anisotropic=True)], None, ("coord",)),
    "carried_box": ("box", 129, 18, [dict(type="CenterShift", apply_z=True), dict(type="RandomScale", scale=[0.5, 2.0], anisotropic=True),
                                     dict(type="RandomFlip", p=1.0), dict(type="RandomShift"), _rot("y", None),
                                     dict(type="CenterShift", apply_z=False)], None, ("coord", "normal")),
    "jitter_both_clips": ("box", 129, 19, [dict(type="RandomJitter", sigma=0.05, clip=0.05)], None, ("coord",)),
    "point_clip": ("box", 129, 20, [dict(type="PointClip", point_cloud_range=(3.5, -1.5, 1.25, 6.0, 0.5, 3.0))], None, ("coord",)),
    "color_jitter_saturates": ("box", 129, 21, [dict(type="ChromaticJitter", p=1.0, std=0.5)], None, ("color",)),
    "color_translation": ("box", 129, 22, [dict(type="ChromaticTranslation", p=1.0, ratio=0.5)], None, ("color",)),
    "autocontrast_given_blend": ("const_channel", 129, 23, [dict(type="ChromaticAutoContrast", p=1.0, blend_factor=0.5)], None, ("color",)),
    "autocontrast_drawn_blend": ("box", 129, 24, [dict(type="ChromaticAutoContrast", p=1.0)], None, ("color",)),
    "autocontrast_constant": ("const_color", 129, 25, [dict(type="ChromaticAutoContrast", p=1.0, blend_factor=0.5)], None, ("color",)),
    "color_ops_then_normalize": ("box", 129, 26, [dict(type="ChromaticTranslation", p=1.0), dict(type="ChromaticAutoContrast", p=1.0),
                                                  dict(type="ChromaticJitter", p=1.0, std=0.05), dict(type="NormalizeColor")], None, ("color",)),
    "elastic_lattice": ("lattice", 129, 27, [dict(type="ElasticDistortion", distortion_params=[[0.25, 0.4]])], dict(random=[0.1]), ("coord",)),
    "elastic_flat": ("flat", 129, 28, [dict(type="ElasticDistortion", distortion_params=[[0.7, 0.4]])], dict(random=[0.1]), ("coord",)),
    "elastic_one_point": ("box", 1, 29, [dict(type="ElasticDistortion", distortion_params=[[0.2, 0.4]])], dict(random=[0.1]), ("coord",)),
    "elastic_two_stages": ("box", 129, 30, [dict(type="ElasticDistortion")], dict(random=[0.1]), ("coord",)),
    "elastic_after_affine": ("box", 129, 31, [_rot("z", [0, 0, 0]), dict(type="RandomScale"), dict(type="ElasticDistortion"),
                                              dict(type="CenterShift", apply_z=True)], dict(random=[0.1, 0.1]), ("coord", "normal")),
    "chain_one_point": ("box", 1, 32, SCANNET_CHAIN, ONE_POINT_FORCED, POINT_KEYS),
    "chain_affine_tile_plus_one": ("box", TILE + 1, 33, SCANNET_CHAIN[:7], dict(random=[0.1] * 4, rand=[0.2, 0.7]), ("coord", "normal")),
    "chain_scannet_two_tiles_plus_one": ("box", 2 * TILE + 1, 34, SCANNET_CHAIN, CHAIN_FORCED, POINT_KEYS),
}
ELASTIC_GRIDS = {"elastic_lattice": [(5, 6, 4)], "elastic_flat": [(8, 7, 3)], "elastic_one_point": [(3, 3, 3)]}

_golden = {}


def golden():
    if not _golden:
        _golden.update(np.load(GOLDEN))
    return _golden


def recorded(name):
    """-> per transform of the case the list of (function, value) the reference drew"""
    g, out = golden(), []
    for ti in range(len(CASES[name][3])):
        row, j = [], 0
        while True:
            hit = [k for k in g if k.startswith(f"{name}/t{ti}/r{j}/")]
            if not hit:
                break
            row.append((hit[0].rsplit("/", 1)[1], g[hit[0]]))
            j += 1
        out.append(row)
    return out


def to_draw(cfg, rec, device):
    """the recorded values of one reference transform -> the draw= of its port"""
    kind = cfg["type"]
    vals = [v for _, v in rec]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)       # noqa: E731
    if kind in ("RandomRotate", "RandomRotateTargetAngle"):
        return dict(gate=float(vals[0]), **(dict(angle=float(vals[1])) if len(vals) > 1 else {}))
    if kind == "RandomShift":
        return dict(shift=[float(v) for v in vals])
    if kind == "RandomScale":
        return dict(scale=np.asarray(vals[0], dtype=np.float64))
    if kind == "RandomFlip":
        return dict(x=float(vals[0]), y=float(vals[1]))
    if kind == "RandomJitter":
        return dict(noise=t(vals[0].astype(np.float32)))
    if kind == "ElasticDistortion":
        return dict(gate=float(vals[0]), noise=[t(v.astype(np.float32)) for v in vals[1:]])
    if kind == "ChromaticAutoContrast":
        return dict(gate=float(vals[0]), **(dict(blend=float(vals[1])) if len(vals) > 1 else {}))
    if kind == "ChromaticTranslation":
        return dict(gate=float(vals[0]), **(dict(tr=vals[1].reshape(3)) if len(vals) > 1 else {}))
    if kind == "ChromaticJitter":
        return dict(gate=float(vals[0]), **(dict(noise=t(vals[1].astype(np.float32))) if len(vals) > 1 else {}))
    if kind == "RandomDropout":
        return dict(gate=float(vals[0]), **(dict(index=t(vals[1].astype(np.int64))) if len(vals) > 1 else {}))
    assert not vals, (kind, rec)
    return None


def load_case(name, device):
    """-> (config list, input dict on `device`, draws, golden outputs {key: float64 array})"""
    kind, n, seed, cfg, _, keys = CASES[name]
    sc = scene(kind, n, seed)
    g = golden()
    assert float(g[f"{name}/checksum"]) == float(sum(sc[k].astype(np.float64).sum() for k in POINT_KEYS)), "scene() changed: regenerate the golden"
    draws = [to_draw(c, r, device) for c, r in zip(cfg, recorded(name))]
    data = {k: torch.from_numpy(v).to(device) for k, v in sc.items()}
    return cfg, data, draws, {k: g[f"{name}/out/{k}"] for k in keys}


def _err(t, gold):
    return float(np.abs(t.detach().cpu().numpy().astype(np.float64) - gold).max())


_figures = {}


def check_case(device, name, kernels=None):
    """fused Compose and the transforms called one by one, same draws, both against the golden with the twin's error as the bound"""
    cfg, data, draws, gold = load_case(name, device)
    fused = AUG.Compose(cfg, force_kernels=kernels)(dict(data), draws)
    twin = AUG.Compose(cfg, force_kernels=False)(dict(data), draws)
    single = dict(data)
    for c, d in zip(cfg, draws):
        tr = AUG.Compose([c], force_kernels=kernels).transforms[0]
        tr.force_kernels = kernels
        single = tr(single, d)
    for k in POINT_KEYS:             # the inputs are never modified
        assert torch.equal(data[k], torch.from_numpy(scene(*CASES[name][:3])[k]).to(device))
    for key, gd in gold.items():
        assert fused[key].dtype == torch.float32 and tuple(fused[key].shape) == gd.shape, (name, key, fused[key].shape, gd.shape)
        scale = max(float(np.abs(gd).max()), float(data[key].abs().max()))
        e_twin, e_fused, e_single = _err(twin[key], gd), _err(fused[key], gd), _err(single[key], gd)
        bound = max(2 * e_twin, 2.0 ** -23 * float(np.abs(gd).max()))
        twin_bound = 16 * 2.0 ** -24 * scale * len(cfg)
        _figures[(name, key)] = (e_fused, e_single, e_twin, bound, twin_bound)
        print(f"{name:34s} {key:6s} engine fused {e_fused:.3e} one by one {e_single:.3e} twin {e_twin:.3e} bound {bound:.3e} "
              f"twin bound {twin_bound:.3e}")
        assert e_twin <= twin_bound, (name, key, e_twin, twin_bound)
        assert e_fused <= bound and e_single <= bound, (name, key, e_fused, e_single, bound)
    if "coord" in gold:
        assert fused["segment"].shape[0] == fused["coord"].shape[0] == gold["coord"].shape[0]
    return fused


def parity_table(device, kernels=None):
    lines = [f"{'case':34s} {'key':6s} {'engine fused':>12s} {'one by one':>12s} {'fp32 twin':>12s} {'bound':>12s} {'twin bound':>12s}"]
    for name in CASES:
        check_case(device, name, kernels)
        for (nm, key), f in _figures.items():
            if nm == name:
                lines.append(f"{name:34s} {key:6s} " + " ".join(f"{v:12.3e}" for v in f))
    return "\n".join(lines)


def check_rotated_box_is_told_apart():
    """rotate_then_rotate_box: the centre of the ROTATED FIRST BOX and the centre of the box of the rotated cloud differ by far more than
    any bound of check_case, so an engine that carried the box through the rotation cannot pass"""
    name = "rotate_then_rotate_box"
    kind, n, seed, cfg, _, _ = CASES[name]
    c = scene(kind, n, seed)["coord"].astype(np.float64)
    a = float(recorded(name)[0][1][1]) * np.pi
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rotated = c @ R.T
    true_centre = (rotated.min(0) + rotated.max(0)) / 2
    carried = ((c.min(0) + c.max(0)) / 2) @ R.T
    assert np.abs(true_centre - carried).max() > 0.1


def check_elastic_grid_shapes():
    for name, shapes in ELASTIC_GRIDS.items():
        got = [tuple(v.shape[:3]) for fn, v in recorded(name)[0][1:]]
        assert got == shapes, (name, got)
    assert len(recorded("elastic_two_stages")[0]) == 3


def check_gate_false(device, kernels=None):
    """every p-gate closed: the outputs are the inputs' values bit for bit"""
    sc = {k: torch.from_numpy(v).to(device) for k, v in scene("box", TILE + 1, 40).items()}
    cfg = [dict(type="RandomDropout", dropout_application_ratio=0.2), dict(type="RandomRotate", p=0.5), dict(type="RandomRotateTargetAngle"),
           dict(type="RandomFlip", p=0.5), dict(type="ElasticDistortion"), dict(type="ChromaticAutoContrast"), dict(type="ChromaticTranslation"),
           dict(type="ChromaticJitter")]
    draws = [dict(gate=0.5), dict(gate=0.9), dict(gate=0.9), dict(x=0.7, y=0.5), dict(gate=0.99), dict(gate=0.5), dict(gate=0.99), dict(gate=0.99)]
    out = AUG.Compose(cfg, force_kernels=kernels)(dict(sc), draws)
    for k in sc:
        assert torch.equal(out[k], sc[k]), k
    for c, d in zip(cfg, draws):
        tr = AUG.Compose([c]).transforms[0]
        tr.force_kernels = kernels
        out = tr(dict(sc), d)
        for k in sc:
            assert torch.equal(out[k], sc[k]), (c["type"], k)


def check_empty_chain_and_coord_only(device, kernels=None):
    sc = {k: torch.from_numpy(v).to(device) for k, v in scene("box", 300, 41).items()}
    out = AUG.Compose([], force_kernels=kernels)(dict(sc))
    assert all(torch.equal(out[k], sc[k]) for k in sc)
    only = dict(coord=sc["coord"])
    cfg = [dict(type="CenterShift"), _rot("z", None), dict(type="RandomFlip", p=1.0), dict(type="ChromaticAutoContrast", p=1.0),
           dict(type="ChromaticJitter", p=1.0), dict(type="NormalizeColor"), dict(type="RandomJitter"), dict(type="ElasticDistortion")]
    draws = [None, dict(gate=0.0, angle=0.3), None, None, None, None, dict(seed=5), dict(gate=0.0, seed=7)]
    a = AUG.Compose(cfg, force_kernels=kernels)(dict(only), draws)
    assert sorted(a) == ["coord"] and a["coord"].shape == sc["coord"].shape and bool(torch.isfinite(a["coord"]).all())
    # a dict without any point key passes through
    assert AUG.Compose(cfg[:3], force_kernels=kernels)(dict(name="scene0"), draws[:3]) == dict(name="scene0")
    # normals without coordinates: rotated and flipped about nothing
    nrm = AUG.Compose(cfg[1:3], force_kernels=kernels)(dict(normal=sc["normal"]), draws[1:3])["normal"]
    ref = AUG.Compose(cfg[1:3], force_kernels=False)(dict(normal=sc["normal"]), draws[1:3])["normal"]
    assert float((nrm - ref).abs().max()) <= 2.0 ** -22


def check_conversions(device, kernels=None):
    """float64 and non-contiguous inputs are converted; outputs are fp32"""
    sc = scene("box", 300, 42)
    wide = torch.from_numpy(np.concatenate([sc["coord"], sc["coord"]], 1).astype(np.float64)).to(device)
    data = dict(coord=wide[:, :3], color=torch.from_numpy(sc["color"]).to(device).to(torch.float64))
    cfg = [dict(type="CenterShift"), dict(type="NormalizeColor")]
    out = AUG.Compose(cfg, force_kernels=kernels)(data)
    ref = AUG.Compose(cfg, force_kernels=False)(dict(coord=torch.from_numpy(sc["coord"]).to(device), color=torch.from_numpy(sc["color"]).to(device)))
    assert out["coord"].dtype == out["color"].dtype == torch.float32 and out["coord"].is_contiguous()
    assert float((out["coord"] - ref["coord"]).abs().max()) <= 2.0 ** -21
    # the kernel divides by 255; torch's division by a scalar multiplies by the rounded reciprocal on the GPU: one ulp of values <= 1
    assert float((out["color"] - ref["color"]).abs().max()) <= 2.0 ** -23


def check_determinism(device, kernels=None):
    """the same seed twice is bit-identical, two seeds differ, and the noise of a point does not depend on n"""
    big = {k: torch.from_numpy(v).to(device) for k, v in scene("box", 2 * TILE + 1, 43).items()}
    small = {k: v[:TILE + 1].clone() for k, v in big.items()}
    for cfg, key in ((dict(type="RandomJitter", sigma=0.01, clip=0.05), "coord"), (dict(type="ChromaticJitter", p=1.0, std=0.05), "color")):
        tr = AUG.Compose([cfg]).transforms[0]
        tr.force_kernels = kernels
        a, b, c = tr(dict(big), dict(gate=0.0, seed=11))[key], tr(dict(big), dict(gate=0.0, seed=11))[key], tr(dict(big), dict(gate=0.0, seed=12))[key]
        assert torch.equal(a, b) and not torch.equal(a, c), cfg["type"]
        assert float((a - big[key]).abs().max()) > 0
        p = tr(dict(small), dict(gate=0.0, seed=11))[key]
        assert torch.equal(p, a[:TILE + 1]), cfg["type"]
    tr = AUG.Compose([dict(type="ElasticDistortion")]).transforms[0]
    tr.force_kernels = kernels
    a, b, c = (tr(dict(small), dict(gate=0.0, seed=s))["coord"] for s in (21, 21, 22))
    assert torch.equal(a, b) and not torch.equal(a, c)
    full = AUG.Compose(SCANNET_CHAIN, force_kernels=kernels)
    torch.manual_seed(5)
    draws = [None] * len(SCANNET_CHAIN)
    draws[1] = dict(gate=0.9)                   # the dropout's permutation comes from torch's generator: leave it out
    import random

    outs = []
    for _ in range(2):
        random.seed(3), np.random.seed(3), torch.manual_seed(3)
        outs.append(full(dict(small), draws))
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in POINT_KEYS)


def check_generator(device, kernels=None):
    """N = 65 536 samples per stream and component: six-sigma bounds of the estimators"""
    N = 65536
    for stream in (ops.AUG_STREAM_JITTER, ops.AUG_STREAM_COLOR, ops.AUG_STREAM_ELASTIC):
        z = ops.aug_noise(1234567, stream, 3 * N, device).double().reshape(N, 3).cpu()
        mean, var = z.mean(0), z.var(0, unbiased=False)
        zc = (z - mean) / var.sqrt()
        corr = [float((zc[:, i] * zc[:, j]).mean()) for i, j in ((0, 1), (0, 2), (1, 2))]
        print(f"stream {stream}: mean {mean.tolist()} var {var.tolist()} corr {corr}")
        assert float(mean.abs().max()) < 6 / N ** 0.5
        assert float((var - 1).abs().max()) < 6 * (2 / N) ** 0.5
        assert max(abs(c) for c in corr) < 6 / N ** 0.5
        assert bool(torch.isfinite(z).all())
    a, b = ops.aug_noise(7, 0, 1000, device), ops.aug_noise(7, 0, 3000, device)
    assert torch.equal(a, b[:1000]) and not torch.equal(a, ops.aug_noise(7, 1, 1000, device)) and not torch.equal(a, ops.aug_noise(8, 0, 1000, device))


def check_refusals(device, kernels=None):
    for name in ("MultiViewGenerator", "ContrastiveViewsGenerator", "HueSaturationTranslation", "RandomColorJitter", "RandomColorGrayScale",
                 "RandomDropColor", "RandomDropNormal", "ClipGaussianJitter", "NormalizeCoord", "PositiveShift", "InstanceParser", "Update",
                 "ImgAugmentation"):
        with pytest.raises(PtcoreError, match=name):
            AUG.Compose([dict(type="CenterShift"), dict(type=name)])
    with pytest.raises(PtcoreError, match="object"):
        AUG.Compose([object()])
    empty = dict(coord=torch.zeros((0, 3), device=device), color=torch.zeros((0, 3), device=device))
    for cfg in ([dict(type="CenterShift")], [dict(type="ElasticDistortion")], []):
        with pytest.raises(PtcoreError, match="empty point cloud"):
            AUG.Compose(cfg, force_kernels=kernels)(dict(empty))
    tr = AUG.RandomJitter()
    tr.force_kernels = kernels
    with pytest.raises(PtcoreError, match="empty point cloud"):
        tr(dict(empty))
    with pytest.raises(PtcoreError, match=r"noise of shape"):
        e = AUG.ElasticDistortion([[0.25, 0.4]])
        e.force_kernels = kernels
        e(dict(coord=torch.from_numpy(scene("lattice", 64, 1)["coord"]).to(device)), dict(gate=0.0, noise=[torch.zeros(5, 7, 4, 3, device=device)]))
    with pytest.raises(PtcoreError, match="draws"):
        AUG.Compose([dict(type="CenterShift")], force_kernels=kernels)(dict(coord=torch.zeros((4, 3), device=device)), [None, None])


def check_scannet_config_end_to_end(device, kernels=None):
    """the whole training list of configs/scannet/semseg-pt-v3m1-0-base.py: Compose hands over to GridSample / SphereCrop and takes the
    cloud back; compared with the same list run in stages (the augmentations' golden-checked prefix, then each transform alone)"""
    from pointcept_amd import transform as T

    tail = [dict(type="GridSample", grid_size=0.02, hash_type="fnv", mode="train", return_grid_coord=True),
            dict(type="SphereCrop", point_max=600, mode="random"), dict(type="CenterShift", apply_z=False), dict(type="NormalizeColor"),
            dict(type="ToTensor"), dict(type="Collect", keys=("coord", "grid_coord", "segment"), feat_keys=("color", "normal"))]
    cfg, data, draws, _ = load_case("chain_affine_tile_plus_one", device)
    torch.manual_seed(9)                       # GridSample's per-voxel picks come from torch's generator
    out = AUG.Compose(cfg + tail, force_kernels=kernels)(dict(data), draws + [None, 17, None, None, None, None])
    assert sorted(out) == ["coord", "feat", "grid_coord", "offset", "segment"]
    m = out["coord"].shape[0]
    assert m == 600 and out["feat"].shape == (m, 6) and out["grid_coord"].shape == (m, 3) and int(out["offset"][0]) == m
    assert out["coord"].dtype == torch.float32 and float(out["feat"][:, :3].min()) >= 0 and float(out["feat"][:, :3].max()) <= 1
    lo, hi = out["coord"].min(0).values, out["coord"].max(0).values
    assert float((lo[:2] + hi[:2]).abs().max()) <= 2.0 ** -20 * float(hi.abs().max() + 1)       # CenterShift(apply_z=False) came last
    # staged: the same draws, every transform called on its own
    torch.manual_seed(9)
    st = AUG.Compose(cfg, force_kernels=kernels)(dict(data), draws)
    st = T.GridSample(grid_size=0.02, return_grid_coord=True)(st)
    st = T.SphereCrop(point_max=600)(st, center_index=17)
    cs, nc = AUG.CenterShift(apply_z=False), AUG.NormalizeColor()
    cs.force_kernels = nc.force_kernels = kernels
    st = nc(cs(st))
    assert torch.equal(st["grid_coord"], out["grid_coord"]) and torch.equal(st["segment"], out["segment"])
    assert float((st["coord"] - out["coord"]).abs().max()) <= 2.0 ** -22 * float(out["coord"].abs().max())
    assert torch.equal(torch.cat([st["color"], st["normal"]], 1), out["feat"])


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def keep_global_rng():
    """these tests seed and consume python's, numpy's and torch's global generators (the transforms draw from them, as the reference's
    do): every test leaves them as it found them, so the tests that run afterwards see the streams they saw before this file existed"""
    import random

    state = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])
    torch.set_rng_state(state[2])
    if state[3] is not None:
        torch.cuda.set_rng_state_all(state[3])


@pytest.mark.parametrize("name", list(CASES))
def test_case_against_the_reference_golden(name):
    check_case(dev(), name)


def test_golden_cases_are_what_they_claim():
    check_rotated_box_is_told_apart()
    check_elastic_grid_shapes()


def test_closed_gates_leave_the_bits():
    check_gate_false(dev())


def test_empty_chain_coord_only_and_conversions():
    check_empty_chain_and_coord_only(dev())
    check_conversions(dev())


def test_seeds_and_prefix_independence():
    check_determinism(dev())


def test_generator_statistics():
    check_generator(dev())


def test_refusals():
    check_refusals(dev())


def test_scannet_config_end_to_end():
    check_scannet_config_end_to_end(dev())


def test_switch_takes_the_twin(monkeypatch):
    assert config.AUGMENT_KERNELS is True and "PTC_AUGMENT=0" in config.__doc__
    cfg, data, draws, _ = load_case("carried_box", dev())
    monkeypatch.setattr(config, "AUGMENT_KERNELS", False)
    a = AUG.Compose(cfg)(dict(data), draws)
    b = AUG.Compose(cfg, force_kernels=False)(dict(data), draws)
    assert all(torch.equal(a[k], b[k]) for k in POINT_KEYS)
