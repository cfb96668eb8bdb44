"""ctypes binding of libvitamd.so (C ABI declared in include/vitamd.h).

The library is built in-tree by `csrc/Makefile` (see __graft_entry__.build).  There is no
fallback: if it is missing, `load()` raises — the product path never routes around the HIP kernels.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvitamd.so")
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
ABI_VERSION = 9


class VitamdError(RuntimeError):
    pass


HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "vitamd.h")
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong,
            "float": ctypes.c_float, "double": ctypes.c_double}
_TYPE_WORDS = {"void", "char", "short", "int", "long", "float", "double", "signed", "unsigned", "const", "struct"}
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(VITAMD_\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$", re.M)
_DECL = re.compile(r"(?:^|(?<=[;{}]))([^;{}()]*?)\b(vitamd_\w+)\s*\(([^()]*)\)\s*;")


def parse_header(text):
    """The C ABI as include/vitamd.h declares it: ({name: (return type, [parameter type, ...])}, {VITAMD_* macro: int}).  Types are canonical C
    spellings (`const float*`, `unsigned long long`); a pointer to anything, or one of _SCALARS.  Anything else raises, naming the declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {name: int(value, 0) for name, value in _DEFINE.findall(text)}        # object-like macros with an integer body only
    protos = {}
    for ret, name, params in _DECL.findall(re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)):
        ret = " ".join(ret.split())
        if ret not in ("int", "long"):
            raise VitamdError(f"{name}: return type `{ret}` is not int or long")
        types = []
        for param in ([] if params.strip() in ("", "void") else params.split(",")):
            words = [w for w in param.replace("*", " * ").split() if w != "__restrict__"]
            if len(words) < 2 or words[-1] in _TYPE_WORDS or not re.fullmatch(r"[A-Za-z_]\w*", words[-1]):
                raise VitamdError(f"{name}: parameter `{' '.join(param.split())}` has no name")
            ctype = " ".join(words[:-1]).replace(" *", "*")
            if not ctype.endswith("*") and ctype not in _SCALARS:
                raise VitamdError(f"{name}: no ctypes type for parameter `{' '.join(param.split())}`")
            types.append(ctype)
        protos[name] = (ret, types)
    return protos, constants


try:
    with open(HEADER) as _fh:
        PROTOTYPES, CONSTANTS = parse_header(_fh.read())
except OSError as _e:
    raise VitamdError(f"{HEADER} is missing: the binding is derived from it") from _e
SIGNATURES = {name: [ctypes.c_void_p if t.endswith("*") else _SCALARS[t] for t in types] for name, (_, types) in PROTOTYPES.items()}      # name -> argtypes
RESTYPES = {name: _SCALARS[ret] for name, (ret, _) in PROTOTYPES.items()}
# include/vitamd_eval.h: the evaluation entry points added beside ABI 9 (the tables above stay those of vitamd.h alone); its limits join CONSTANTS
EVAL_HEADER = os.path.join(os.path.dirname(HEADER), "vitamd_eval.h")
try:
    with open(EVAL_HEADER) as _fh:
        EVAL_PROTOTYPES, _eval_constants = parse_header(_fh.read())
except OSError as _e:
    raise VitamdError(f"{EVAL_HEADER} is missing: the binding is derived from it") from _e
CONSTANTS.update(_eval_constants)
EVAL_SIGNATURES = {name: [ctypes.c_void_p if t.endswith("*") else _SCALARS[t] for t in types] for name, (_, types) in EVAL_PROTOTYPES.items()}
EVAL_RESTYPES = {name: _SCALARS[ret] for name, (ret, _) in EVAL_PROTOTYPES.items()}
ERRORS = {CONSTANTS["VITAMD_ERR_SHAPE"]: "unsupported shape", CONSTANTS["VITAMD_ERR_ARG"]: "bad argument",
          CONSTANTS["VITAMD_ERR_LAUNCH"]: "HIP launch failure", CONSTANTS["VITAMD_ERR_INIT"]: "vitamd_init has not run for this device"}

_lib = None


def build(verbose: bool = False) -> str:
    """Compile libvitamd.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode != 0:
        raise VitamdError("building libvitamd.so failed")
    return LIB_PATH


def hip_runtimes(maps_path="/proc/self/maps"):
    """The distinct libamdhip64 files mapped into this process (by real path)."""
    found = set()
    with open(maps_path) as fh:
        for line in fh:
            parts = line.split(None, 5)
            if len(parts) == 6 and "libamdhip64" in os.path.basename(parts[5].strip()):
                found.add(os.path.realpath(parts[5].strip()))
    return sorted(found)


def check_single_hip_runtime(maps_path="/proc/self/maps"):
    """Two HIP runtimes in one process - e.g. /opt/rocm's libamdhip64 pulled in by an early dlopen of libvitamd.so AND the copy a PyTorch wheel
    bundles - register kernels with one and pass streams and pointers of the other: the first launch fails with `HIP launch failure` (round 3,
    gpurun_out/r3/smoke_dbg*.log).  Detected here instead of relying on import order: raises VitamdError naming both files."""
    found = hip_runtimes(maps_path)
    if len(found) > 1 and os.environ.get("VITAMD_ALLOW_TWO_HIP_RUNTIMES") != "1":      # (the variable: for a tool that maps a second copy it never launches through)
        raise VitamdError("two HIP runtimes are mapped into this process: " + " and ".join(found) + " - libvitamd.so must resolve libamdhip64 to "
                          "the runtime that owns the caller's streams and pointers (import torch / load the framework BEFORE dlopen-ing libvitamd.so)")
    return found


def load():
    """Load the library (once) and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VitamdError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the HIP kernels are the only implementation of this path; there is no fallback)")
    # torch FIRST: its wheel bundles its own HIP runtime (libamdhip64.so of the ROCm it was built against).  Loaded before torch, libvitamd.so would pull
    # /opt/rocm's copy in and torch then its own: two HIP runtimes in one process - kernels registered with one, streams and pointers from the other -
    # and the first launch fails (seen on a GPU box with `build(); smoke()` in one process).  With torch imported first the library's libamdhip64
    # dependency resolves to the runtime already in the process.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    check_single_hip_runtime()
    for signatures, restypes in ((SIGNATURES, RESTYPES), (EVAL_SIGNATURES, EVAL_RESTYPES)):
        for name, argtypes in signatures.items():
            fn = getattr(lib, name)  # AttributeError here = header/library mismatch
            fn.argtypes = argtypes
            fn.restype = restypes[name]
    if lib.vitamd_abi_version() != ABI_VERSION:
        raise VitamdError("libvitamd.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        raise VitamdError(f"{what}: {ERRORS.get(code, code)}")
