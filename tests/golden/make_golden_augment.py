"""Generate tests/golden/augment.npz by running the REFERENCE'S OWN transform classes (pointcept/datasets/transform.py, imported
unmodified) on float64 copies of the seeded scenes of tests/test_gpu_augment.py (CASES / scene()).  Only runnable where the reference
tree exists; the .npz output is committed.

    python tests/golden/make_golden_augment.py

float64 copies: the reference then computes in one precision throughout (on float32 input it switches to float64 at the first applied
rotation).  Every value that random.random and np.random.uniform / rand / randn / choice return while a transform runs is recorded --
randn's values are rounded to fp32 first, so that the reference itself computes with the noise the engine is given -- and saved per
transform as <case>/t<i>/r<j>/<function>; a case's `forced` scalars are handed out by random.random / the scalar rand() in order, so
that a chain's gates open as the case wants.  Saved per case: a float64 checksum of the inputs (the tests regenerate them from the seed
and compare), the recorded draws and the outputs of the compared keys in float64.  Data only: no reference code is stored.
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("POINTCEPT_REFERENCE", "/root/reference")


def load_reference_transforms():
    """pointcept/datasets/transform.py as a module of its own: its registry and torchvision imports are satisfied by stubs (the image
    transforms that use torchvision are never constructed)"""
    if "ref_transform" in sys.modules:
        return sys.modules["ref_transform"]
    sys.dont_write_bytecode = True

    class Registry:
        def __init__(self, name):
            self.name = name

        def register_module(self, *a, **k):
            return lambda cls: cls

    stubs = {"pointcept": dict(__path__=[]), "pointcept.utils": dict(__path__=[]), "pointcept.utils.registry": dict(Registry=Registry)}
    try:
        import torchvision  # noqa: F401
    except ImportError:
        stubs["torchvision"] = dict(transforms=types.ModuleType("torchvision.transforms"))
    before = {name: sys.modules.get(name) for name in stubs}
    for name, attrs in stubs.items():          # for the duration of the import only: other tests import the real packages
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    try:
        spec = importlib.util.spec_from_file_location("ref_transform", os.path.join(REF, "pointcept", "datasets", "transform.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name, old in before.items():
            if old is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = old
    sys.modules["ref_transform"] = mod
    return mod


class Recorder:
    """patches random.random and np.random.uniform / rand / randn / choice; .log holds (function, value) of the calls since clear()"""

    def __init__(self, forced=None):
        forced = forced or {}
        self.forced = {k: list(v) for k, v in forced.items()}
        self.log = []
        self.saved = []

    def _wrap(self, owner, name, tag):
        orig = getattr(owner, name)

        def f(*a, **k):
            if tag in ("random", "rand") and not a and self.forced.get(tag):
                v = self.forced[tag].pop(0)
            else:
                v = orig(*a, **k)
            if tag == "randn":
                v = np.asarray(v).astype(np.float32).astype(np.float64)
            self.log.append((tag, np.asarray(v).copy()))
            return v

        self.saved.append((owner, name, orig))
        setattr(owner, name, f)

    def __enter__(self):
        self._wrap(random, "random", "random")
        for name in ("uniform", "rand", "randn", "choice"):
            self._wrap(np.random, name, name)
        return self

    def __exit__(self, *exc):
        for owner, name, orig in self.saved:
            setattr(owner, name, orig)
        assert not any(self.forced.values()), f"forced draws left over: {self.forced}"


def run_reference(ref, cfg, sc, forced, seed):
    """-> (outputs dict of float64 arrays, per transform the recorded draws)"""
    data = {k: (v.astype(np.float64) if v.dtype == np.float32 else v.copy()) for k, v in sc.items()}
    random.seed(seed)
    np.random.seed(seed)
    rows = []
    with Recorder(forced) as rec:
        for c in cfg:
            c = dict(c)
            t = getattr(ref, c.pop("type"))(**c)
            rec.log = []
            data = t(data)
            rows.append(list(rec.log))
    return data, rows


def main():
    import test_gpu_augment as A

    ref = load_reference_transforms()
    out = {}
    for name, (kind, n, seed, cfg, forced, keys) in A.CASES.items():
        sc = A.scene(kind, n, seed)
        data, rows = run_reference(ref, cfg, sc, forced, seed)
        out[f"{name}/checksum"] = np.float64(sum(sc[k].astype(np.float64).sum() for k in A.POINT_KEYS))
        for ti, row in enumerate(rows):
            for j, (fn, v) in enumerate(row):
                v = v.astype(np.float32) if fn == "randn" else v
                out[f"{name}/t{ti}/r{j}/{fn}"] = v
        for k in keys:
            assert data[k].dtype == np.float64, (name, k, data[k].dtype)
            out[f"{name}/out/{k}"] = data[k]
        print(f"{name:34s} n {n:5d} -> {data['coord'].shape[0]:5d} draws {[len(r) for r in rows]}")
    path = os.path.join(OUT, "augment.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
