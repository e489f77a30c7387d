"""Host cost of one C-ABI call through the binding (profiles/abi_binding.txt), four forms in alternating repeats in one process:
  (a) `check(raw.ptc_x(...), "ptc_x")` on the raw handle, the handle hoisted       (b) `lib().ptc_x(...)` on the checked handle, the
  call site of today (the status raised by a ctypes errcheck)       (c) `check(lib(checked=False).ptc_x(...), "ptc_x")`, the call site
  of before as it was written, lib() paid per call       (d) `C.ptc_x(...)`, the checked function with the handle hoisted.
(d) against (a) is the errcheck against check(); (b) against (c) is the two call sites like for like.  The call is ptc_rope3d_xyz with
n = 0: thirteen arguments, returns PTC_OK before any launch, so the time is the binding's.  Needs no GPU (the library loads without one).

    python tools/abi_binding_time.py [--calls 200000] [--repeats 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch  # noqa: F401  (its import is not the binding's)

    t0 = time.perf_counter()
    from pointcept_amd import _lib                      # reads and parses include/ptcore.h
    t_import = time.perf_counter() - t0
    t0 = time.perf_counter()
    _lib.parse_header(open(_lib.HEADER_PATH).read())
    t_parse = time.perf_counter() - t0
    t0 = time.perf_counter()
    _lib.lib()                                          # build() finds the library up to date, CDLL, two views bound
    t_first = time.perf_counter() - t0
    from pointcept_amd._lib import check, lib

    raw = lib(checked=False)
    a = (None, 2, None, 2, None, None, 0, 3, 2, 4, 18, 1.0, None)

    C = lib()

    def wrapped(k):           # (a)
        for _ in range(k):
            check(raw.ptc_rope3d_xyz(*a), "ptc_rope3d_xyz")

    def checked(k):           # (b)
        for _ in range(k):
            lib().ptc_rope3d_xyz(*a)

    def wrapped_lib(k):       # (c) the call site of before as it was written, lib() paid per call
        for _ in range(k):
            check(lib(checked=False).ptc_rope3d_xyz(*a), "ptc_rope3d_xyz")

    def checked_hoisted(k):   # (d) the errcheck alone against check() of (a)
        for _ in range(k):
            C.ptc_rope3d_xyz(*a)

    forms = (("a", wrapped), ("b", checked), ("c", wrapped_lib), ("d", checked_hoisted))
    for _, f in forms:
        f(20000)
    ns = {name: [] for name, _ in forms}
    for _ in range(args.repeats):
        for name, f in forms:
            t0 = time.perf_counter()
            f(args.calls)
            ns[name].append((time.perf_counter() - t0) / args.calls * 1e9)
    med = {k: statistics.median(v) for k, v in ns.items()}
    rng = {k: max(v) - min(v) for k, v in ns.items()}
    label = {"a": "(a) check(raw.ptc_rope3d_xyz(...), name)           ", "b": "(b) lib().ptc_rope3d_xyz(...)  [checked]           ",
             "c": "(c) check(lib(checked=False).ptc_rope3d_xyz(...), name)", "d": "(d) C.ptc_rope3d_xyz(...)  [checked, C = lib()]     "}

    def holds(x, y):
        return f"median ({x}) {med[x]:.1f} <= median ({y}) + range ({y}) = {med[y] + rng[y]:.1f}: " + ("holds" if med[x] <= med[y] + rng[y] else "DOES NOT HOLD")

    ok = med["b"] <= med["a"] + rng["a"]
    lines = [f"per-call host cost of ptc_rope3d_xyz(n = 0), {args.repeats} alternating repeats of {args.calls} calls, ns per call"]
    lines += ["  " + label[k] + "  " + " ".join(f"{v:7.1f}" for v in ns[k]) + f"   median {med[k]:.1f}  range {rng[k]:.1f}" for k in "abcd"]
    lines += [
        "  required: " + holds("b", "a"),
        "  the parts: errcheck against check(), handle hoisted: " + holds("d", "a"),
        "             the checked call site against the call site of before with its lib(): " + holds("b", "c"),
        f"first use (for information): import of the package after torch's {t_import * 1e3:.1f} ms, of which one parse of "
        f"include/ptcore.h {t_parse * 1e3:.2f} ms ({len(_lib.HEADER.signatures)} declarations); first lib() {t_first * 1e3:.1f} ms",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        open(args.out, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
