"""Generate tests/golden/lovasz_wide.npz by running the REFERENCE'S OWN LovaszLoss(mode="multiclass", ignore_index=-1)
(pointcept/models/losses/lovasz.py, imported unmodified through oracle/ref_import.py) in fp32 on the seeded cases of
tests/test_gpu_lovasz_wide.py (GOLDEN_CASES, built on oracle.ptv3_model.lovasz_case): 65..200 classes of which only some occur.
Only runnable where the reference tree exists; the .npz output is committed.

    python tests/golden/make_golden_lovasz_wide.py

Stored per case, with the discipline of lovasz.npz (tests/golden/make_golden.py): the case's parameters, the labels and a float64
checksum of the logits (the tests regenerate both from the seed and compare), the reference's loss and its gradient w.r.t. the logits.
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle import ref_import  # noqa: E402


def load_reference_lovasz():
    ref_import.load()
    if "pointcept.models.losses" not in sys.modules:
        pkg = types.ModuleType("pointcept.models.losses")
        pkg.__path__ = [ref_import.REF + "/pointcept/models/losses"]
        sys.modules["pointcept.models.losses"] = pkg
    return importlib.import_module("pointcept.models.losses.lovasz")


def run_reference(lov, x, y):
    """-> (loss, gradient [n, c] fp32) of the reference module"""
    crit = lov.LovaszLoss(mode="multiclass", ignore_index=-1, loss_weight=1.0)
    x = x.clone().requires_grad_(True)
    loss = crit(x, y)
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def main():
    from test_gpu_lovasz_wide import GOLDEN_CASES, GOLDEN_PRESENT, wide_case

    lov = load_reference_lovasz()
    blobs = {}
    for ci, spec in enumerate(GOLDEN_CASES):
        x, y = wide_case(*spec)
        assert len(np.unique(y.numpy()[y.numpy() >= 0])) == GOLDEN_PRESENT[ci], (ci, len(np.unique(y.numpy()[y.numpy() >= 0])))
        loss, grad = run_reference(lov, x, y)
        blobs[f"spec_{ci}"] = np.asarray(spec[:6], dtype=np.float64)
        blobs[f"mode_{ci}"] = np.asarray(spec[6])
        blobs[f"logits_sum_{ci}"], blobs[f"labels_{ci}"] = np.asarray(float(x.double().sum())), y.numpy().astype(np.int16)
        blobs[f"loss_{ci}"], blobs[f"grad_{ci}"] = np.asarray(loss), grad
    blobs["n_cases"] = np.asarray(len(GOLDEN_CASES))
    path = os.path.join(OUT, "lovasz_wide.npz")
    np.savez_compressed(path, **blobs)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
