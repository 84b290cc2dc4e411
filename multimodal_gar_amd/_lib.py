"""ctypes binding of libmgar_hip.so -- the ONLY way the Python host code reaches the kernels.

The product path has no CPU fallback: if the HIP library is missing this module raises at
import time, and every op refuses non-device tensors.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmgar_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "mgar_ops.h")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "multimodal_gar_amd: %s is missing -- build it with `python -m multimodal_gar_amd.build` "
        "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
if not os.path.exists(HEADER_PATH):
    raise ImportError(
        "multimodal_gar_amd: %s is missing -- the bindings are read from it (the package runs from "
        "its repository tree)." % HEADER_PATH)

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}


def _header_int(text, name):
    """Value of `#define <name> <n>` in the text of include/mgar_ops.h (None if absent)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    m = re.search(r"^#define %s (\d+)\s*$" % re.escape(name), text, flags=re.M)
    return int(m.group(1)) if m else None


def _parse_header(text):
    """(MGAR_ABI_VERSION, {name: (restype, [argtypes])}) of every mgar_* declaration in the text of include/mgar_ops.h.
    Strict on purpose: int / float / double / long long, pointers (void *) and a `const char *` result are all the ABI
    uses; a declaration with anything else raises instead of binding as something plausible."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    version = _header_int(text, "MGAR_ABI_VERSION")
    if version is None:
        raise ImportError("mgar_ops.h: no `#define MGAR_ABI_VERSION <n>`")
    text = re.sub(r'^[ \t]*#[^\n]*|extern\s+"C"\s*\{|\}', " ", text, flags=re.M)
    protos = {}
    for decl in filter(None, (" ".join(d.replace("*", " * ").split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.+?) ?\b(mgar_\w+) ?\(([^()]*)\)", decl)
        if not m:
            raise ImportError("mgar_ops.h: cannot parse `%s`" % decl)
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        restype = ctypes.c_char_p if ret == "const char *" else _SCALARS.get(ret)
        argtypes = []
        for param in ([] if params == "void" else params.split(",")):
            words = param.split()
            argtypes.append(ctypes.c_void_p if "*" in words else _SCALARS.get(" ".join(words[:-1])))  # last word: the name
        if restype is None or None in argtypes or name in protos:
            raise ImportError("mgar_ops.h: unsupported type or duplicate in `%s`" % decl)
        protos[name] = (restype, argtypes)
    return version, protos


with open(HEADER_PATH) as _f:
    _header = _f.read()
ABI_VERSION, _protos = _parse_header(_header)
DAFM_MAX_N = _header_int(_header, "MGAR_DAFM_MAX_N")   # actors per scene the DAFM kernels hold in registers
if DAFM_MAX_N is None:
    raise ImportError("mgar_ops.h: no `#define MGAR_DAFM_MAX_N <n>`")
BF16_TWINS = frozenset(n[:-5] for n in _protos if n.endswith("_bf16"))

_cdll = ctypes.CDLL(LIB_PATH)
_fns = {}
for _name, (_res, _args) in _protos.items():
    _fn = getattr(_cdll, _name)  # AttributeError here = the library is stale: rebuild it
    _fn.restype, _fn.argtypes = _res, _args
    _fns[_name] = _fn

# The bindings and ABI_VERSION both come from the header, so they cannot disagree with each other; what is left to catch
# is a libmgar_hip.so compiled from an older header.
if _fns["mgar_abi_version"]() != ABI_VERSION:
    raise ImportError("libmgar_hip.so ABI %d != expected %d: rebuild" % (_fns["mgar_abi_version"](), ABI_VERSION))


class MgarError(RuntimeError):
    pass


def dev_ptr(t, dtype=None):
    """Raw device pointer of a contiguous device tensor (the C ABI takes nothing else)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise MgarError("expected a device (HIP) tensor, got %s -- there is no CPU path" % t.device)
    if not t.is_contiguous():
        raise MgarError("tensor must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise MgarError("expected dtype %s, got %s" % (dtype, t.dtype))
    return t.data_ptr()


def fptr(t):
    return dev_ptr(t, torch.float32)


def pptr(t, dtype):
    """Pointer of a feature-payload tensor, which must have the payload dtype of the call (float32 or bfloat16)."""
    return dev_ptr(t, dtype)


def payload_call(name, dtype, *args):
    """`name` for float32 payloads, its `_bf16` twin for bfloat16 ones."""
    if dtype == torch.float32:
        return call(name, *args)
    if dtype == torch.bfloat16 and name in BF16_TWINS:
        return call(name + "_bf16", *args)
    raise MgarError("%s: unsupported payload dtype %s" % (name, dtype))


def iptr(t):
    return dev_ptr(t, torch.int32)


def stream_of(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def raw(name, *args):
    """Call an entry point whose return value is not a status code (e.g. a size query)."""
    return _fns[name](*args)


def call(name, *args):
    rc = _fns[name](*args)
    if rc != 0:
        raise MgarError("%s failed with code %d: %s" % (name, rc, _fns["mgar_last_error"]().decode()))
    return rc


def host_arrays(radii, nsamples, idx_tensors):
    """ctypes host arrays (float[], int[], void*[]) for the multi-radius ball query entry points."""
    n = len(radii)
    fa = (ctypes.c_float * n)(*[float(r) for r in radii])
    ia = (ctypes.c_int * n)(*[int(s) for s in nsamples])
    pa = (ctypes.c_void_p * n)(*[iptr(t) for t in idx_tensors])
    return fa, ia, pa


def kernel_timers(enable=None, reset=True):
    """enable=True/False switches the per-kernel HIP-event timers of the library; otherwise returns
    {kernel name: (total_ms, launches, algorithmic_bytes, flops)} since the last reset."""
    if enable is not None:
        call("mgar_ktimer_enable", int(bool(enable)))
        _KT_STATE["on"] = bool(enable)
        return None
    out = {}
    for i in range(raw("mgar_ktimer_count")):
        ms, by, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        call("mgar_ktimer_read", i, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(by), ctypes.byref(fl), int(reset))
        if n.value:
            out[raw("mgar_ktimer_name", i).decode()] = (ms.value, n.value, by.value, fl.value)
    return out


_KT_IDS = {}


_KT_STATE = {"on": False}


def note_work(kernel, flops=0.0, nbytes=0.0):
    """Instrumented runs only: credit algorithmic flops / bytes to `kernel` for launches whose work only the caller knows
    (per-sample counts or pair lists that live on the device)."""
    if not _KT_STATE["on"]:
        return
    if not _KT_IDS:
        for i in range(raw("mgar_ktimer_count")):
            _KT_IDS[raw("mgar_ktimer_name", i).decode()] = i
    if flops:
        call("mgar_ktimer_add_flops", _KT_IDS[kernel], float(flops))
    if nbytes:
        call("mgar_ktimer_add_bytes", _KT_IDS[kernel], float(nbytes))


def kernel_timing_on():
    return _KT_STATE["on"]


def note_pair_tests(kernel, pairs):
    """Instrumented runs only: credit `pairs` (query, point) distance evaluations (8 flop each) to `kernel`."""
    note_work(kernel, flops=float(pairs) * 8.0)


def exported_symbols():
    return sorted(_fns)
