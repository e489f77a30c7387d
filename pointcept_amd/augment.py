"""Device-side point augmentation: the transforms of pointcept/datasets/transform.py that sit between the raw
scene and GridSample in every training config, for point clouds that already live on the GPU.  Same class names, constructor arguments,
defaults and dict protocol as the reference; torch tensors instead of numpy arrays; inputs are never modified.

    CenterShift RandomShift RandomRotate RandomRotateTargetAngle RandomScale RandomFlip     one pending 3 x 4 matrix  ptc_aug_compose
    RandomJitter PointClip NormalizeColor ChromaticAutoContrast / Translation / Jitter      the flush                 ptc_aug_apply
    ElasticDistortion                                                   ptc_aug_elastic_grid + ptc_aug_elastic_apply
    RandomDropout ShufflePoint                                          row selection in torch (transform.index_operator)

The plan (csrc/augment.hip).  A run of affine transforms is not applied: it advances a pending affine (A, t for coordinates, Rn for
normals) that is held on the device in double, and the coordinates are written once, at the next flush.  CenterShift and a RandomRotate
without a centre need the bounding box of the CURRENT cloud: a reduce pass (ptc_aug_reduce) leaves it on the device and the compose
kernel reads it there; the box is carried exactly through shift / scale / flip, so only a rotation or a row selection costs another
reduce.  Row selection commutes with the pending affine and does not flush.  Colour ops ride in whichever flush comes next.

Host reads.  Each ElasticDistortion stage reads its 6-float bounding box once, to size its noise grid (GridSample takes one sync per
scene for the same kind of reason).  Nothing else here synchronises: the scalar draws (gates, angles, scales) are host values as in the
reference, the bounding-box centres stay on the device.

Draws.  Every random class takes `draw=` at call time: a dict of the values the reference would draw, in the reference's own units
(`gate`: the uniform the p-gate compares; `angle`: the uniform before the factor pi; ...; see each class), and for per-point or per-cell
noise either `noise` (the standard-normal tensor itself) or `seed` (the in-kernel generator: a pure function of seed, stream and element
index).  Without it the scalars come from Python's `random` / `numpy.random` as in the reference and the seeds from torch's generator.

config.AUGMENT_KERNELS (PTC_AUGMENT=0) and CPU tensors take the torch twin: the same transforms op by op in fp32, written from the
reference's behaviour (its noise comes from torch's generator seeded with `seed`, not from the kernels' generator).
"""
from __future__ import annotations

import random

import numpy as np
import torch

from . import config as _config
from . import ops
from . import transform as _T
from ._lib import PtcoreError

_POINT_KEYS = ("coord", "normal", "color")


def _seed() -> int:
    return int(torch.randint(0, 2 ** 53, (1,)).item())       # torch's CPU generator: no device work


def _use_kernels(t: torch.Tensor, force) -> bool:
    return bool(_config.AUGMENT_KERNELS and t.is_cuda) if force is None else bool(force)


def _enter(data_dict):
    """a shallow copy with coord / normal / color as contiguous fp32; an empty cloud is refused"""
    data = dict(data_dict)
    n = None
    for key in _POINT_KEYS:
        if key in data:
            t = data[key]
            if not torch.is_tensor(t):
                raise PtcoreError(f"augment: data_dict['{key}'] must be a torch tensor, got {type(t).__name__}")
            if t.shape[0] == 0:
                raise PtcoreError("augment: empty point cloud")
            if t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
                raise PtcoreError(f"augment: data_dict['{key}'] must be [n, 3], got {tuple(t.shape)}")
            n = t.shape[0]
            if t.dtype != torch.float32 or not t.is_contiguous():
                data[key] = t.to(torch.float32).contiguous()
    return data


def _ref(data):
    for key in _POINT_KEYS:
        if key in data:
            return data[key]
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# the planner's state for one scene (kernel path)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Scene:
    def __init__(self, data, want_color_box=False):
        self.data = data
        self.aff = None               # device [21] float64 once something was composed; None: identity
        self.stats = None             # device [12] float64
        self.ops = []                 # descriptors not yet sent to ptc_aug_compose
        self.dirty = False            # the pending affine (sent or not) moves coordinates
        self.dirty_n = False          # ... normals
        self.box = False              # stats[0:6] is the box of the current cloud under everything pending
        self.color_box = False        # stats[6:12] is the channel min / max of data["color"]
        self.color_ops = []
        self.want_color_box = want_color_box
        self.hint_box = False         # the next transform needs the box: a flush leaves it behind
        self.launches = 0             # op-wrapper calls (tools/augment_step.py)

    def _state(self):
        if self.stats is None:
            self.stats = torch.empty(12, dtype=torch.float64, device=_ref(self.data).device)
        return self.stats

    def reduce(self, color=False):
        """the box of the current cloud (and, on request, the colours' min / max) -> stats"""
        self.send()
        coord = None if self.box or "coord" not in self.data else self.data["coord"]
        col = self.data.get("color") if (color or self.want_color_box) and not self.color_box and not self.color_ops else None
        if coord is None and col is None:
            return
        ops.aug_reduce(coord, col, self.aff if self.dirty else None, self._state())
        self.launches += 2
        self.box = self.box or coord is not None
        self.color_box = self.color_box or col is not None

    def push(self, op, needs_box=False, keeps_box=True, normals=False):
        if "coord" not in self.data and not (normals and "normal" in self.data):
            return
        if needs_box and not self.box:
            self.reduce()
        self.ops.append(op)
        self.dirty = True
        self.dirty_n = self.dirty_n or normals
        self.box = self.box and keeps_box

    def send(self):
        if not self.ops:
            return
        fresh = self.aff is None
        if fresh:
            self.aff = torch.empty(21, dtype=torch.float64, device=_ref(self.data).device)
        ops.aug_compose(self.ops, self.aff, self._state(), fresh)
        self.launches += -(-len(self.ops) // ops.AUG_MAX_OPS)
        self.ops = []

    def select(self, index):
        """row selection: commutes with the pending affine; the boxes are those of another cloud afterwards"""
        self.data = _T.index_operator(self.data, index)
        self.box = self.color_box = False

    def flush(self, coord=True, jitter=None, clip_range=None):
        """materialise: everything pending is written once.  coord=False keeps the pending coordinates for a consumer that applies the
        affine itself (the elastic kernel) and writes normals and colours only."""
        self.send()
        d = self.data
        if any(op[0] == ops.AUG_C_AUTOCONTRAST for op in self.color_ops) and not self.color_box:
            raise PtcoreError("augment: internal error, ChromaticAutoContrast was planned without its colour statistics")
        c_in = d.get("coord") if coord and (self.dirty or jitter is not None or clip_range is not None) else None
        n_in = d.get("normal") if self.dirty_n else None
        k_in = d.get("color") if self.color_ops else None
        want_stats = c_in is not None and self.hint_box
        if c_in is not None or n_in is not None or k_in is not None:
            stats = self._state() if want_stats else self.stats
            c, nrm, k = ops.aug_apply(c_in, n_in, k_in, self.aff if (self.dirty or self.dirty_n) else None, stats, jitter, clip_range,
                                      self.color_ops if k_in is not None else (), want_stats)
            self.launches += 2 if want_stats else 1
            if c is not None:
                d["coord"] = c
            if nrm is not None:
                d["normal"] = nrm
            if k is not None:
                d["color"] = k
                self.color_box = False
        self.color_ops = []
        self.dirty_n = False
        if coord:
            if c_in is not None:
                self.box = want_stats
            self.aff, self.dirty = None, False

    def consumed(self):
        """a kernel applied the pending coordinates itself: the pending affine is the identity afterwards"""
        self.aff, self.dirty, self.dirty_n = None, False, False


class _Transform:
    """Base of the ported transforms: __call__(data_dict, draw=None) works alone (own launches, correct result); Compose calls
    plan(scene, drawn) on the kernel path and twin(data, drawn) on the torch path with the same drawn values."""
    force_kernels = None        # tests: True runs the kernels whatever the device (the host emulation)
    wants_box = False

    def drawn(self, data, draw):
        return draw or {}

    def plan(self, scene, drawn):
        raise NotImplementedError

    def twin(self, data, drawn):
        raise NotImplementedError

    @torch.no_grad()
    def __call__(self, data_dict, draw=None):
        data = _enter(data_dict)
        ref = _ref(data)
        drawn = self.drawn(data, draw)
        if ref is None:
            return data
        if not _use_kernels(ref, self.force_kernels):
            return self.twin(data, drawn)
        scene = _Scene(data, want_color_box=isinstance(self, ChromaticAutoContrast))
        self.plan(scene, drawn)
        scene.flush()
        return scene.data


def _vec(values, like):
    return torch.tensor([float(v) for v in values], dtype=torch.float64).to(device=like.device, dtype=like.dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# affine transforms
# ---------------------------------------------------------------------------------------------------------------------------------
class CenterShift(_Transform):
    """transform.py:172-185"""
    wants_box = True

    def __init__(self, apply_z=True):
        self.apply_z = apply_z

    def plan(self, scene, drawn):
        scene.push((ops.AUG_CENTER_SHIFT, 1.0 if self.apply_z else 0.0), needs_box=True)

    def twin(self, data, drawn):
        if "coord" in data:
            c = data["coord"]
            lo, hi = c.min(0).values, c.max(0).values
            shift = torch.stack([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, lo[2] if self.apply_z else torch.zeros_like(lo[2])])
            data["coord"] = c - shift
        return data


class RandomShift(_Transform):
    """transform.py:189-199.  draw: shift = the three uniforms"""

    def __init__(self, shift=((-0.2, 0.2), (-0.2, 0.2), (0, 0))):
        self.shift = shift

    def drawn(self, data, draw):
        d = dict(draw or {})
        if "shift" not in d and "coord" in data:
            d["shift"] = [np.random.uniform(self.shift[i][0], self.shift[i][1]) for i in range(3)]
        return d

    def plan(self, scene, drawn):
        if "coord" in scene.data:
            scene.push((ops.AUG_SHIFT, *[float(v) for v in drawn["shift"]]))

    def twin(self, data, drawn):
        if "coord" in data:
            data["coord"] = data["coord"] + _vec(drawn["shift"], data["coord"])
        return data


_AXES = {"x": 0, "y": 1, "z": 2}


def _rotation(axis, angle):
    c, s = np.cos(angle), np.sin(angle)          # transform.py:260-268
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    if axis == "z":
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    raise NotImplementedError


class RandomRotate(_Transform):
    """transform.py:241-281.  draw: gate (applied unless gate > p), angle (the uniform of [angle[0], angle[1]], before the factor pi)"""

    def __init__(self, angle=None, center=None, axis="z", always_apply=False, p=0.5):
        self.angle = [-1, 1] if angle is None else angle
        self.axis = axis
        self.always_apply = always_apply
        self.p = p if not self.always_apply else 1
        self.center = center
        self.wants_box = center is None

    def _angle(self):
        return np.random.uniform(self.angle[0], self.angle[1])

    def drawn(self, data, draw):
        d = dict(draw or {})
        if "gate" not in d:
            d["gate"] = random.random()
        d["apply"] = not d["gate"] > self.p
        if d["apply"] and "angle" not in d:
            d["angle"] = self._angle()
        return d

    def plan(self, scene, drawn):
        if not drawn["apply"]:
            return
        if self.axis not in _AXES:
            raise NotImplementedError
        angle = drawn["angle"] * np.pi
        given = self.center is not None
        centre = [float(v) for v in self.center] if given else [0.0, 0.0, 0.0]
        has_coord = "coord" in scene.data
        scene.push((ops.AUG_ROTATE, _AXES[self.axis], float(np.cos(angle)), float(np.sin(angle)), 1.0 if given or not has_coord else 0.0,
                    *centre), needs_box=has_coord and not given, keeps_box=False, normals=True)

    def twin(self, data, drawn):
        if not drawn["apply"]:
            return data
        rot = _rotation(self.axis, drawn["angle"] * np.pi)
        if "coord" in data:
            c = data["coord"]
            rot_t = torch.from_numpy(rot.T.copy()).to(device=c.device, dtype=c.dtype)
            centre = (c.min(0).values + c.max(0).values) / 2 if self.center is None else _vec(self.center, c)
            data["coord"] = (c - centre) @ rot_t + centre
        if "normal" in data:
            nrm = data["normal"]
            data["normal"] = nrm @ torch.from_numpy(rot.T.copy()).to(device=nrm.device, dtype=nrm.dtype)
        return data


class RandomRotateTargetAngle(RandomRotate):
    """transform.py:285-320.  draw: gate, angle (the chosen entry of `angle`, before the factor pi)"""

    def __init__(self, angle=(1 / 2, 1, 3 / 2), center=None, axis="z", always_apply=False, p=0.75):
        super().__init__(angle=angle, center=center, axis=axis, always_apply=always_apply, p=p)

    def _angle(self):
        return np.random.choice(self.angle)


class RandomScale(_Transform):
    """transform.py:324-335.  draw: scale (one uniform, three when anisotropic)"""

    def __init__(self, scale=None, anisotropic=False):
        self.scale = scale if scale is not None else [0.95, 1.05]
        self.anisotropic = anisotropic

    def drawn(self, data, draw):
        d = dict(draw or {})
        if "scale" not in d and "coord" in data:
            d["scale"] = np.random.uniform(self.scale[0], self.scale[1], 3 if self.anisotropic else 1)
        if "scale" in d:
            s = [float(v) for v in np.atleast_1d(np.asarray(d["scale"], dtype=np.float64))]
            d["scale"] = s * 3 if len(s) == 1 else s
        return d

    def plan(self, scene, drawn):
        if "coord" in scene.data:
            scene.push((ops.AUG_SCALE, *drawn["scale"]))

    def twin(self, data, drawn):
        if "coord" in data:
            data["coord"] = data["coord"] * _vec(drawn["scale"], data["coord"])
        return data


class RandomFlip(_Transform):
    """transform.py:339-354.  draw: x, y (the two uniforms; an axis flips when its value < p)"""

    def __init__(self, p=0.5):
        self.p = p

    def drawn(self, data, draw):
        d = dict(draw or {})
        for k in ("x", "y"):
            if k not in d:
                d[k] = np.random.rand()
        d["flip"] = (bool(d["x"] < self.p), bool(d["y"] < self.p))
        return d

    def plan(self, scene, drawn):
        fx, fy = drawn["flip"]
        if fx or fy:
            scene.push((ops.AUG_FLIP, float(fx), float(fy)), normals=True)

    def twin(self, data, drawn):
        for axis, on in enumerate(drawn["flip"]):
            if on:
                for key in ("coord", "normal"):
                    if key in data:
                        t = data[key].clone()
                        t[:, axis] = -t[:, axis]
                        data[key] = t
        return data


# ---------------------------------------------------------------------------------------------------------------------------------
# transforms that write coordinates
# ---------------------------------------------------------------------------------------------------------------------------------
def _noise(drawn, shape, device, generator_seed_offset=0):
    """the twin's standard-normal noise: the injected tensor, else torch's generator seeded with the draw's seed"""
    if drawn.get("noise") is not None:
        return drawn["noise"].to(device=device, dtype=torch.float32)
    g = torch.Generator(device="cpu").manual_seed(int(drawn["seed"]) + generator_seed_offset)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(device)


class RandomJitter(_Transform):
    """transform.py:358-372.  draw: noise ([n, 3] standard normal) or seed"""

    def __init__(self, sigma=0.01, clip=0.05):
        assert clip > 0
        self.sigma = sigma
        self.clip = clip

    def drawn(self, data, draw):
        d = dict(draw or {})
        if d.get("noise") is None and "seed" not in d:
            d["seed"] = _seed()
        return d

    def plan(self, scene, drawn):
        if "coord" in scene.data:
            scene.flush(jitter=(self.sigma, self.clip, drawn.get("noise"), drawn.get("seed", 0)))

    def twin(self, data, drawn):
        if "coord" in data:
            c = data["coord"]
            data["coord"] = c + torch.clamp(self.sigma * _noise(drawn, c.shape, c.device), -self.clip, self.clip)
        return data


class PointClip(_Transform):
    """transform.py:203-214"""

    def __init__(self, point_cloud_range=(-80, -80, -3, 80, 80, 1)):
        self.point_cloud_range = point_cloud_range

    def plan(self, scene, drawn):
        if "coord" in scene.data:
            scene.flush(clip_range=[float(v) for v in self.point_cloud_range])

    def twin(self, data, drawn):
        if "coord" in data:
            c = data["coord"]
            data["coord"] = torch.minimum(torch.maximum(c, _vec(self.point_cloud_range[:3], c)), _vec(self.point_cloud_range[3:], c))
        return data


def _grid_dims(box6, granularity):
    """transform.py:796-799 on the 6-float box (the host read of an elastic stage): the box is that of the fp32 points"""
    b = np.asarray(box6, dtype=np.float64).astype(np.float32).astype(np.float64)
    return [int(v) + 3 for v in (b[3:6] - b[0:3]) // granularity]


def _blur_twin(noise):
    """two rounds of width-3 box filters along x, y, z with zero padding (transform.py:793-812), fp32"""
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32, device=noise.device)
    for _ in range(2):
        for axis in range(3):
            pad = torch.zeros_like(noise.narrow(axis, 0, 1))
            p = torch.cat([pad, noise, pad], dim=axis)
            m = noise.shape[axis]
            noise = p.narrow(axis, 0, m) * third + p.narrow(axis, 1, m) * third + p.narrow(axis, 2, m) * third
    return noise


class ElasticDistortion(_Transform):
    """transform.py:779-836.  draw: gate (applied when gate < 0.95), noise (one [dx, dy, dz, 3] standard-normal tensor per stage, the
    grid shape being floor(extent / granularity) + 3 per axis) or seed.  One host read of the 6-float bounding box per stage."""
    wants_box = True

    def __init__(self, distortion_params=None):
        self.distortion_params = [[0.2, 0.4], [0.8, 1.6]] if distortion_params is None else distortion_params

    def drawn(self, data, draw):
        d = dict(draw or {})
        if "coord" in data and self.distortion_params is not None:
            if "gate" not in d:
                d["gate"] = random.random()
            d["apply"] = bool(d["gate"] < 0.95)
            if d["apply"] and d.get("noise") is None and "seed" not in d:
                d["seed"] = _seed()
        else:
            d["apply"] = False
        return d

    def plan(self, scene, drawn):
        if not drawn["apply"]:
            return
        if scene.dirty_n or scene.color_ops:
            scene.flush(coord=False)
        for s, (granularity, magnitude) in enumerate(self.distortion_params):
            scene.reduce()
            box = scene.stats[:6].cpu().numpy()                  # the host read of this stage
            dims = _grid_dims(box, granularity)
            noise = drawn["noise"][s] if drawn.get("noise") is not None else None
            grid = ops.aug_elastic_grid(dims, noise, drawn.get("seed", 0), ops.AUG_STREAM_ELASTIC + s, scene.data["coord"].device)
            scene.data["coord"] = ops.aug_elastic_apply(scene.data["coord"], scene.aff if scene.dirty else None, scene.stats, grid,
                                                        granularity, magnitude)
            scene.launches += 3 + (noise is None)
            scene.consumed()
            scene.box = True

    def twin(self, data, drawn):
        if not drawn["apply"]:
            return data
        c = data["coord"]
        for s, (granularity, magnitude) in enumerate(self.distortion_params):
            lo, hi = c.min(0).values, c.max(0).values
            dims = _grid_dims(torch.cat([lo, hi]).cpu().numpy(), granularity)
            if drawn.get("noise") is not None:
                noise = drawn["noise"][s].to(device=c.device, dtype=torch.float32)
                if list(noise.shape) != dims + [3]:
                    raise PtcoreError(f"ElasticDistortion: noise of shape {tuple(noise.shape)} for a grid of {tuple(dims + [3])}")
            else:
                noise = _noise(drawn, dims + [3], c.device, s)
            grid = _blur_twin(noise)
            g = torch.tensor(granularity, dtype=torch.float32, device=c.device)
            u = (c - (lo - g)) / g
            cell = torch.minimum(torch.clamp(torch.floor(u), min=0).long(), torch.tensor(dims, device=c.device) - 2)
            f = u - cell.to(u.dtype)
            out = torch.zeros_like(c)
            for ox in (0, 1):
                for oy in (0, 1):
                    for oz in (0, 1):
                        w = (f[:, 0] if ox else 1 - f[:, 0]) * (f[:, 1] if oy else 1 - f[:, 1]) * (f[:, 2] if oz else 1 - f[:, 2])
                        out = out + w[:, None] * grid[cell[:, 0] + ox, cell[:, 1] + oy, cell[:, 2] + oz]
            c = c + out * magnitude
        data["coord"] = c
        return data


# ---------------------------------------------------------------------------------------------------------------------------------
# colour
# ---------------------------------------------------------------------------------------------------------------------------------
class _Color(_Transform):
    p = 1.0

    def drawn(self, data, draw):
        d = dict(draw or {})
        d["apply"] = False
        if "color" in data:
            if "gate" not in d:
                d["gate"] = np.random.rand()
            d["apply"] = bool(d["gate"] < self.p)
        return d


class ChromaticAutoContrast(_Color):
    """transform.py:397-422.  draw: gate (applied when gate < p), blend (the uniform, when blend_factor is None)"""

    def __init__(self, p=0.2, blend_factor=None):
        self.p = p
        self.blend_factor = blend_factor

    def drawn(self, data, draw):
        d = super().drawn(data, draw)
        if d["apply"]:
            d["blend"] = float(self.blend_factor) if self.blend_factor is not None else float(d["blend"]) if "blend" in d else np.random.rand()
        return d

    def plan(self, scene, drawn):
        if not drawn["apply"]:
            return
        if scene.color_ops:                 # lo / hi are those of the colours as this op meets them
            scene.flush()
        scene.reduce(color=True)
        scene.color_ops.append((ops.AUG_C_AUTOCONTRAST, drawn["blend"], 0.0, 0.0, None, 0, 0))

    def twin(self, data, drawn):
        if not drawn["apply"]:
            return data
        c = data["color"]
        lo, hi = c.min(0, keepdim=True).values, c.max(0, keepdim=True).values
        diff = hi - lo
        scale = torch.where(diff > 0, 255 / torch.where(diff > 0, diff, torch.ones_like(diff)), torch.ones_like(diff))
        b = drawn["blend"]
        out = (1 - b) * c + b * ((c - lo) * scale)
        data["color"] = torch.where((diff > 0).any(), out, c)
        return data


class ChromaticTranslation(_Color):
    """transform.py:426-435.  draw: gate, tr (the three uniforms of [0, 1))"""

    def __init__(self, p=0.95, ratio=0.05):
        self.p = p
        self.ratio = ratio

    def drawn(self, data, draw):
        d = super().drawn(data, draw)
        if d["apply"]:
            tr = np.asarray(d["tr"], dtype=np.float64).reshape(3) if "tr" in d else np.random.rand(1, 3).reshape(3)
            d["shift"] = [float(v) for v in (tr - 0.5) * 255 * 2 * self.ratio]
        return d

    def plan(self, scene, drawn):
        if drawn["apply"]:
            scene.color_ops.append((ops.AUG_C_TRANSLATION, *drawn["shift"], None, 0, 0))

    def twin(self, data, drawn):
        if drawn["apply"]:
            c = data["color"]
            data["color"] = torch.clamp(_vec(drawn["shift"], c) + c, 0, 255)
        return data


class ChromaticJitter(_Color):
    """transform.py:439-451.  draw: gate, noise ([n, 3] standard normal) or seed"""

    def __init__(self, p=0.95, std=0.005):
        self.p = p
        self.std = std

    def drawn(self, data, draw):
        d = super().drawn(data, draw)
        if d["apply"] and d.get("noise") is None and "seed" not in d:
            d["seed"] = _seed()
        return d

    def plan(self, scene, drawn):
        if drawn["apply"]:
            scene.color_ops.append((ops.AUG_C_JITTER, self.std * 255, 0.0, 0.0, drawn.get("noise"), drawn.get("seed", 0), ops.AUG_STREAM_COLOR))

    def twin(self, data, drawn):
        if drawn["apply"]:
            c = data["color"]
            data["color"] = torch.clamp(_noise(drawn, c.shape, c.device) * torch.tensor(self.std * 255, dtype=c.dtype, device=c.device) + c, 0, 255)
        return data


class NormalizeColor(_Transform):
    """transform.py:143-147"""

    def plan(self, scene, drawn):
        if "color" in scene.data:
            scene.color_ops.append((ops.AUG_C_NORMALIZE, 0.0, 0.0, 0.0, None, 0, 0))

    def twin(self, data, drawn):
        if "color" in data:
            data["color"] = data["color"] / 255
        return data


# ---------------------------------------------------------------------------------------------------------------------------------
# row selection (torch on either path)
# ---------------------------------------------------------------------------------------------------------------------------------
class RandomDropout(_Transform):
    """transform.py:218-237.  draw: gate (applied when gate < dropout_application_ratio), index (the kept rows).  Without a draw the
    rows are a random permutation's head from torch's generator."""

    def __init__(self, dropout_ratio=0.2, dropout_application_ratio=0.5):
        self.dropout_ratio = dropout_ratio
        self.dropout_application_ratio = dropout_application_ratio

    def drawn(self, data, draw):
        d = dict(draw or {})
        if "gate" not in d:
            d["gate"] = random.random()
        d["apply"] = bool(d["gate"] < self.dropout_application_ratio)
        if d["apply"]:
            coord = data["coord"]
            n = coord.shape[0]
            idx = d["index"] if "index" in d else torch.randperm(n)[:int(n * (1 - self.dropout_ratio))]
            idx = torch.as_tensor(idx).to(device=coord.device, dtype=torch.int64)
            if "sampled_index" in data:                      # transform.py:230-235
                idx = torch.unique(torch.cat([idx, data["sampled_index"].to(idx.dtype)]))
                mask = torch.zeros(data["segment"].shape[0], dtype=torch.bool, device=idx.device)
                mask[data["sampled_index"]] = True
                d["sampled_index"] = torch.where(mask[idx])[0]
            d["index"] = idx
        return d

    def _select(self, data, drawn):
        if "sampled_index" in drawn:
            data["sampled_index"] = drawn["sampled_index"]
        return _T.index_operator(data, drawn["index"])

    def plan(self, scene, drawn):
        if drawn["apply"]:
            if "sampled_index" in drawn:
                scene.data["sampled_index"] = drawn["sampled_index"]
            scene.select(drawn["index"])

    def twin(self, data, drawn):
        return self._select(data, drawn) if drawn["apply"] else data


class ShufflePoint(_Transform):
    """transform.py:1061-1067.  draw: index (the permutation)"""

    def drawn(self, data, draw):
        d = dict(draw or {})
        assert "coord" in data
        coord = data["coord"]
        idx = d["index"] if "index" in d else torch.randperm(coord.shape[0])
        d["index"] = torch.as_tensor(idx).to(device=coord.device, dtype=torch.int64)
        return d

    def plan(self, scene, drawn):
        scene.select(drawn["index"])

    def twin(self, data, drawn):
        return _T.index_operator(data, drawn["index"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the pieces of a config's transform list that are not augmentations
# ---------------------------------------------------------------------------------------------------------------------------------
class Copy:
    """transform.py:84-98"""

    def __init__(self, keys_dict=None):
        self.keys_dict = dict(coord="origin_coord", segment="origin_segment") if keys_dict is None else keys_dict

    def __call__(self, data_dict):
        import copy

        for key, value in self.keys_dict.items():
            data_dict[value] = data_dict[key].clone().detach() if torch.is_tensor(data_dict[key]) else copy.deepcopy(data_dict[key])
        return data_dict


class ToTensor:
    """transform.py:115-139: nothing to do for a dict of tensors"""

    def __call__(self, data_dict):
        return data_dict


class Collect:
    """transform.py:54-80: the listed keys, `offset` (one scene: its point count), and name_keys=(...) concatenated as float
    features.  (The reference's line 67 computes a throw-away data_dict["offset"] from the rows of coord; not reproduced.)"""

    def __init__(self, keys, offset_keys_dict=None, **kwargs):
        self.keys = keys
        self.offset_keys = dict(offset="coord") if offset_keys_dict is None else offset_keys_dict
        self.kwargs = kwargs

    def __call__(self, data_dict):
        data = dict()
        keys = [self.keys] if isinstance(self.keys, str) else self.keys
        for key in keys:
            data[key] = data_dict[key]
        for key, value in self.offset_keys.items():
            data[key] = torch.tensor([data_dict[value].shape[0]], device=data_dict[value].device)
        for name, feat_keys in self.kwargs.items():
            name = name.replace("_keys", "")
            assert isinstance(feat_keys, (list, tuple))
            data[name] = torch.cat([data_dict[key].float() for key in feat_keys], dim=1)
        return data


_PLANNED = {c.__name__: c for c in (CenterShift, RandomShift, RandomRotate, RandomRotateTargetAngle, RandomScale, RandomFlip, RandomJitter,
                                    PointClip, ElasticDistortion, ChromaticAutoContrast, ChromaticTranslation, ChromaticJitter,
                                    NormalizeColor, RandomDropout, ShufflePoint)}
_PLAIN = {"GridSample": _T.GridSample, "SphereCrop": _T.SphereCrop, "Copy": Copy, "ToTensor": ToTensor, "Collect": Collect}
_DRAW_KEYWORD = {"GridSample": "rand", "SphereCrop": "center_index"}


class Compose:
    """A config's `transform=[...]` list (config dicts with `type`, or transform objects) on device tensors.  Runs of affine transforms
    become one compose launch with a reduce before each transform that needs the bounding box, colour ops ride in the next flush, and
    everything pending is flushed before a transform that needs materialised data (ElasticDistortion, GridSample, SphereCrop, Copy,
    Collect) and at the end.  A `type` that is not ported is refused by name.

    __call__(data_dict, draws=None): `draws` is a list aligned with the transforms (None entries: drawn as usual); the entry of a
    GridSample is its `rand`, of a SphereCrop its `center_index`."""

    def __init__(self, cfg=None, force_kernels=None):
        self.force_kernels = force_kernels
        self.transforms = []
        for t in (cfg if cfg is not None else []):
            if isinstance(t, dict):
                kw = dict(t)
                name = kw.pop("type", None)
                cls = _PLANNED.get(name) or _PLAIN.get(name)
                if cls is None:
                    raise PtcoreError(f"Compose: transform type '{name}' is not ported to the device front end (ported: "
                                      f"{', '.join(sorted(list(_PLANNED) + list(_PLAIN)))})")
                t = cls(**kw)
            elif not isinstance(t, tuple(_PLANNED.values()) + tuple(_PLAIN.values())):
                raise PtcoreError(f"Compose: transform type '{type(t).__name__}' is not ported to the device front end")
            self.transforms.append(t)
        self.last_launches = 0

    @torch.no_grad()
    def __call__(self, data_dict, draws=None):
        draws = list(draws) if draws is not None else [None] * len(self.transforms)
        if len(draws) != len(self.transforms):
            raise PtcoreError(f"Compose: {len(draws)} draws for {len(self.transforms)} transforms")
        data = _enter(data_dict)
        ref = _ref(data)
        kernels = ref is not None and _use_kernels(ref, self.force_kernels)
        scene = _Scene(data, want_color_box=any(isinstance(t, ChromaticAutoContrast) for t in self.transforms)) if kernels else None
        for i, (t, draw) in enumerate(zip(self.transforms, draws)):
            if isinstance(t, _Transform):
                if ref is None:
                    continue
                live = scene.data if kernels else data
                drawn = t.drawn(live, draw)
                if kernels:
                    nxt = self.transforms[i + 1] if i + 1 < len(self.transforms) else None
                    scene.hint_box = bool(getattr(nxt, "wants_box", False))
                    t.plan(scene, drawn)
                else:
                    data = t.twin(data, drawn)
                continue
            if kernels:
                scene.hint_box = False
                scene.flush()
                data = scene.data
            kw = {} if draw is None else {_DRAW_KEYWORD[type(t).__name__]: draw}
            data = t(data, **kw)
            if kernels:
                if not isinstance(data, dict):           # GridSample(mode="test") returns a list of parts: nothing can follow it here
                    if i + 1 < len(self.transforms):
                        raise PtcoreError("Compose: a transform that returns a list of parts must come last")
                    self.last_launches = scene.launches
                    return data
                launches = scene.launches
                scene = _Scene(_enter(data), want_color_box=scene.want_color_box)
                scene.launches = launches
        if kernels:
            scene.hint_box = False
            scene.flush()
            self.last_launches = scene.launches
            return scene.data
        return data
