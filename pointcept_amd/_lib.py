"""ctypes binding of libptcore.so, derived from include/ptcore.h (the C-ABI's one definition).

(The ptc_aug_* entry points of csrc/augment.hip are declared in csrc/ptcore_augment.h, which is read the same way.)
The header is read once, at import: its declarations give every entry point's restype / argtypes and whether it
returns a status, its enums and integer #defines give the constants (PTC_F32 ..., REDUCE_CODES, ORDER_CODES,
block_enums()).  Nothing of the header is written out a second time here; the parser raises on a declaration it
does not understand.  `lib()` is the CHECKED handle: a status-returning entry point (an `int` one whose last
parameter is the stream) raises PtcoreError with ptc_last_error()'s message instead of returning a non-zero
code, so a call site is `lib().ptc_x(...)`.  `lib(checked=False)` is the RAW handle: the same functions
returning their status integers (`check(rc, name)` raises for those who want it).

`import torch` happens BEFORE the library is loaded so that libptcore.so's DT_NEEDED
libamdhip64.so.7 resolves to the HIP runtime bundled with PyTorch-ROCm (one runtime, shared device
pointers and streams).  There is no CPU fallback: `lib()` raises if the library cannot be loaded,
and every op wrapper in this package raises on non-CUDA tensors.
"""
from __future__ import annotations

import collections
import ctypes
import os
import re
import types
import zlib

import torch  # noqa: F401  (must precede CDLL: provides the HIP runtime)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libptcore.so")
PROBE_PATH = os.path.join(HERE, "libptcore_hostprobe.so")
HEADER_PATH = os.path.normpath(os.path.join(HERE, "..", "include", "ptcore.h"))
AUGMENT_HEADER_PATH = os.path.join(HERE, "csrc", "ptcore_augment.h")      # the augmentation section of the C-ABI, a header of its own

c_i64, c_int, c_f32, c_size, c_ptr = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p


class PtcoreError(RuntimeError):
    """.code: the PTC_E* status of the failing entry point (None for an error raised on the Python side)"""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


# ---- include/ptcore.h -> signatures and constants ------------------------------------------------------------------
_SCALARS = {"int": c_int, "int64_t": c_i64, "size_t": c_size, "uint64_t": ctypes.c_uint64, "float": c_f32, "double": ctypes.c_double}
_RETURNS = {"const char*": ctypes.c_char_p, "int64_t": c_i64, "size_t": c_size, "int": c_int}
_DECL = re.compile(r"(const char\*|int64_t|size_t|int)\s+(ptc_\w+)\s*\(([^()]*)\)")

# signatures: name -> (restype, argtypes, is_status);  enums: tag -> {enumerator: value} (anonymous enums under "");
# constants: every enumerator and every `#define NAME <int>`
Header = collections.namedtuple("Header", "signatures enums constants")


def _is_stream(param: str) -> bool:
    return param.replace("const ", "").split()[0] == "ptc_stream_t"


def parse_header(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    constants = {name: int(val, 0) for name, val in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\w+)[ \t]*$", text, flags=re.M)
                 if re.fullmatch(r"-?(0[xX][0-9a-fA-F]+|\d+)", val)}
    enums = {}
    for tag, body in re.findall(r"\benum\s*(\w*)\s*\{([^}]*)\}", text):
        value = 0
        for item in filter(None, (x.strip() for x in body.split(","))):
            name, _, init = (p.strip() for p in item.partition("="))
            try:
                value = int(init, 0) if init else value
            except ValueError:
                raise PtcoreError(f"include/ptcore.h: enumerator `{item}` is not an integer literal") from None
            enums.setdefault(tag, {})[name] = constants[name] = value
            value += 1
    signatures = {}
    for stmt in re.split(r"[;{}]", re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)):
        stmt = " ".join(stmt.split())
        if not re.search(r"\bptc_\w+\s*\(", stmt):
            continue
        m = _DECL.fullmatch(stmt)
        if m is None or m.group(2) in signatures:
            raise PtcoreError(f"include/ptcore.h: cannot bind the declaration `{stmt}` (return type const char* / int64_t / size_t / "
                              "int, one declaration per name)")
        ret, name, params = m.groups()
        params = [p.strip() for p in params.split(",") if p.strip() not in ("", "void")]
        argtypes = []
        for p in params:
            words = p.replace("const ", "").split()
            base = " ".join(words[:-1]) or words[0]
            if "*" in p or _is_stream(p):
                argtypes.append(c_ptr)
            elif base in _SCALARS:
                argtypes.append(_SCALARS[base])
            else:   # a by-value struct, `long`, ...: nothing the table maps
                raise PtcoreError(f"include/ptcore.h: parameter `{p}` of `{stmt}` has a type this binding does not map")
        # the header's rule (ERRORS): an int entry point whose last parameter is the stream returns a status
        signatures[name] = (_RETURNS[ret], argtypes, ret == "int" and bool(params) and _is_stream(params[-1]))
    return Header(signatures, enums, constants)


def _read_header(path=HEADER_PATH):
    try:
        raw = open(path, "rb").read()
    except OSError as e:
        raise PtcoreError(f"cannot read {path} (the C-ABI's definition; this binding is derived from it): {e}") from e
    return parse_header(raw.decode()), f"{zlib.crc32(raw) & 0xffffffff:08x}"


HEADER, HEADER_CRC = _read_header()
# csrc/ptcore_augment.h: the ptc_aug_* entry points, bound by bind() beside the header's; HEADER stays include/ptcore.h alone
AUGMENT_HEADER = _read_header(AUGMENT_HEADER_PATH)[0]
# name -> (restype, argtypes): the computed table under the name of the literal it replaces.  Nothing in this tree reads it; it is
# what a binder written against that literal reads (tests/emu_backend.py as it was before bind() existed still works on this package)
_SIGNATURES = {name: (restype, argtypes) for name, (restype, argtypes, _) in HEADER.signatures.items()}

PTC_F32, PTC_F16, PTC_BF16 = (HEADER.enums["ptc_dtype"][k] for k in ("PTC_F32", "PTC_F16", "PTC_BF16"))
DTYPE_CODES = {torch.float32: PTC_F32, torch.float16: PTC_F16, torch.bfloat16: PTC_BF16}
REDUCE_CODES = {k[len("PTC_REDUCE_"):].lower(): v for k, v in HEADER.enums["ptc_reduce"].items()}                    # "sum": 0, ...
ORDER_CODES = {k[len("PTC_ORDER_"):].lower().replace("_", "-"): v for k, v in HEADER.enums["ptc_order"].items()}     # "z-trans": 1, ...
_BLK_ENUMS = {k[len("PTC_BLK_"):]: v for k, v in HEADER.constants.items() if k.startswith("PTC_BLK_")}


def exported_symbols():
    return sorted(HEADER.signatures)


def block_enums():
    """name -> index of the PTC_BLK_* argument tables, slabs and slots of ptc_ptv3_block_fwd / _bwd / _layout, and "ABI" -> PTC_BLK_ABI, as include/ptcore.h
    defines them (the header the library was compiled against -- lib() checks its hash)."""
    return _BLK_ENUMS


def bind(cdll, checked: bool, partial: bool = False):
    """A view of `cdll` with one ctypes function per declaration of the header.  checked: the status-returning ones raise
    PtcoreError (message of the same library's ptc_last_error()) instead of returning a non-zero code.  Every view has its own
    function objects (cdll[name]; attribute access on a CDLL would hand out one cached object, and an errcheck set through one
    view would act in the other).  partial: leave out what the library does not export (the host emulation) instead of raising."""
    view = types.SimpleNamespace()
    last_error = cdll["ptc_last_error"]      # the errchecks' own function object: they depend on no view
    last_error.restype, last_error.argtypes = HEADER.signatures["ptc_last_error"][:2]
    for name, (restype, argtypes, is_status) in {**HEADER.signatures, **AUGMENT_HEADER.signatures}.items():
        try:
            fn = cdll[name]
        except AttributeError:   # the library does not export a declared symbol
            if partial:
                continue
            raise
        fn.restype, fn.argtypes = restype, argtypes
        if checked and is_status:
            fn.errcheck = _raiser(name, last_error)
        setattr(view, name, fn)
    return view


def _raiser(name, last_error):
    def errcheck(rc, func, args):
        if rc:
            raise PtcoreError(f"{name} failed with code {rc}: {last_error().decode('utf-8', 'replace')}", rc)
        return rc
    return errcheck


_views = None     # (raw, checked) of libptcore.so once it is loaded


def lib(checked: bool = True):
    """libptcore.so (built first when hipcc is available and the library is missing or stale), bound by bind(): the checked handle
    by default, the raw one (status integers returned) with checked=False."""
    global _views
    if _views is not None:      # the path of every op call
        return _views[checked]
    # build() is mtime-cached (a no-op when nothing changed) and returns the prebuilt library where there is no
    # hipcc (the GPU box): a stale .so can never meet newer ctypes signatures silently
    from . import build as _build

    variant = os.environ.get("PTC_LIB_VARIANT", "")      # compiler-flag A/B builds, see build.VARIANTS
    LIB_PATH = _build.build(variant=variant)
    try:
        cdll = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # fail loudly: no fallback path exists
        raise PtcoreError(f"cannot load {LIB_PATH}: {e}") from e
    raw = bind(cdll, checked=False)
    # ptc_version carries a hash of include/ptcore.h as it was when the library was compiled: compare it with the header this
    # binding was derived from -- equal hashes mean the signatures above are the library's
    m = re.search(r"abi (\w+)", raw.ptc_version().decode())
    got = m.group(1) if m else "none"
    if got != HEADER_CRC:
        raise PtcoreError(f"{LIB_PATH} was built against another include/ptcore.h (abi {got}, header {HEADER_CRC}): rebuild "
                          "(python -m pointcept_amd.build --force)")
    if raw.ptc_aug_abi() != AUGMENT_HEADER.constants["PTC_AUG_ABI"]:
        raise PtcoreError(f"{LIB_PATH} was built against another csrc/ptcore_augment.h (PTC_AUG_ABI {raw.ptc_aug_abi()}, header "
                          f"{AUGMENT_HEADER.constants['PTC_AUG_ABI']}): rebuild (python -m pointcept_amd.build --force)")
    _views = (raw, bind(cdll, checked=True))      # one assignment: another thread sees neither view or both
    return _views[checked]


def check(rc: int, what: str) -> None:
    """for callers of the raw handle: raise what the checked handle raises"""
    if rc != 0:
        msg = lib().ptc_last_error().decode("utf-8", "replace")
        raise PtcoreError(f"{what} failed with code {rc}: {msg}", rc)


def stream_ptr() -> int:
    # the raw HIP stream of torch's current stream on the current device (torch.cuda.current_stream().cuda_stream builds two
    # python objects per call: ~10 us x ~130 calls per step in the round-3 host profile, profiles/r03_i_host_profile.txt)
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def dtype_code(t: torch.Tensor) -> int:
    try:
        return DTYPE_CODES[t.dtype]
    except KeyError:
        raise PtcoreError(f"unsupported feature dtype {t.dtype}") from None


def require_cuda(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise PtcoreError(
                "pointcept_amd ops run only on the GPU through libptcore.so (no CPU fallback); "
                f"got a tensor on {t.device}")


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


# csrc/host_probe.cpp (C++ with function bodies, not a header: its eight signatures are written out)
_PROBES = {
    "probe_serialize_encode": (None, [c_ptr, c_ptr, c_i64, c_int, c_ptr, c_int, c_ptr]),
    "probe_patch_pad_maps": (None, [c_ptr, c_int, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr]),
    "probe_padded_len": (c_i64, [c_i64, c_i64]),
    "probe_num_seq": (c_i64, [c_i64, c_i64]),
    "probe_vox_pack": (ctypes.c_uint64, [c_int, c_int, c_int, c_int]),
    "probe_vox_hash": (ctypes.c_uint64, [ctypes.c_uint64]),
    "probe_voxel_keys": (None, [c_ptr, c_i64, ctypes.c_double, c_ptr, c_ptr, c_ptr]),
    "probe_lovasz_steps": (None, [c_ptr, c_i64, c_ptr]),
}
_probe = None


def host_probe():
    """g++-built copy of the kernels' pure helper functions (CPU unit checks of product code)."""
    global _probe
    if _probe is None:
        if not os.path.exists(PROBE_PATH):
            from . import build as _build

            _build.build_host_probe()
        _probe = ctypes.CDLL(PROBE_PATH)
        for name, (restype, argtypes) in _PROBES.items():
            fn = getattr(_probe, name)
            fn.restype, fn.argtypes = restype, argtypes
    return _probe
